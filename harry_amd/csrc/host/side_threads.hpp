// Threads started beside the caller, owned by one object that joins them on every way out and keeps the first exception any of them
// threw.  The rule it rests on: AN OWNER OF SIDE THREADS IS DECLARED AFTER EVERYTHING ITS THREADS TOUCH (locals, or members of the same
// object), so that its threads are joined before any of that is destroyed.  A thread that waits for its owner's signal (a closing
// flag, a condition variable) gets it before the owner goes; CPU placement, devices and thread budgets stay inside the threads' work.
#pragma once
#include <exception>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace hry {

class SideThreads {
public:
	SideThreads() = default;
	SideThreads(const SideThreads&) = delete;
	SideThreads &operator=(const SideThreads&) = delete;
	~SideThreads() { join(); }   // (never rethrows: an exception already on its way wins)
	// f() on a new thread.  No thread to be had: std::system_error, and the threads started before stay owned
	template <typename F> void spawn(F &&f)
	{
		threads.emplace_back([this, f = std::forward<F>(f)]() mutable {
			try { f(); } catch (...) { std::lock_guard<std::mutex> g(mu); if (!first) first = std::current_exception(); }
		});
	}
	void join() noexcept { for (std::thread &t : threads) t.join(); threads.clear(); }   // every thread spawned so far
	void rethrow() { join(); if (std::exception_ptr e = error()) std::rethrow_exception(e); }
	std::exception_ptr error() const { std::lock_guard<std::mutex> g(mu); return first; }   // the first exception so far, or nullptr

private:
	mutable std::mutex mu;
	std::exception_ptr first;
	std::vector<std::thread> threads;
};

}   // namespace hry
