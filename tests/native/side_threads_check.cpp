// The contract of harry_amd/csrc/host/side_threads.hpp, under ThreadSanitizer and under AddressSanitizer / UBSan.
// Built and run by tests/test_side_threads_cpu.py.  Prints "ok" and exits 0 when every check holds.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../harry_amd/csrc/host/side_threads.hpp"

using hry::SideThreads;

static int failures = 0;
static void check(bool ok, const char *what)
{
	if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}
static void pause_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

int main()
{
	{   // the first of several exceptions is kept; error() sees it before the join
		SideThreads g;
		std::atomic<bool> first_thrown{ false };
		g.spawn([&] { first_thrown = true; throw std::runtime_error("first"); });
		for (int k = 0; k < 3; ++k)
			g.spawn([&] {
				while (!g.error()) std::this_thread::yield();   // (the first one is kept by now)
				throw std::runtime_error("later");
			});
		std::string got;
		try { g.rethrow(); } catch (const std::runtime_error &e) { got = e.what(); }
		check(first_thrown && got == "first", "the first exception is kept");
		std::string again;
		try { g.rethrow(); } catch (const std::runtime_error &e) { again = e.what(); }
		check(again == "first", "rethrow() after a join rethrows the same exception");
	}
	{   // the destructor joins on an exception path, and the caller's exception wins
		std::atomic<bool> finished{ false };
		std::string got;
		try {
			SideThreads g;
			g.spawn([&] { pause_ms(50); finished = true; throw std::runtime_error("side"); });
			throw std::runtime_error("caller");
		} catch (const std::runtime_error &e) {
			got = e.what();
			check(finished.load(), "the destructor joins before the exception reaches its handler");
		}
		check(got == "caller", "the destructor does not rethrow");
	}
	{   // a clean run: rethrow() does nothing; join() twice is harmless; spawn after a join works
		SideThreads g;
		std::vector<int> out(4, 0);
		for (int t = 0; t < 4; ++t) g.spawn([&out, t] { out[t] = t + 1; });
		g.join();
		g.join();
		bool threw = false;
		try { g.rethrow(); } catch (...) { threw = true; }
		check(!threw && g.error() == nullptr, "rethrow() after a clean run does nothing");
		check(out[0] == 1 && out[1] == 2 && out[2] == 3 && out[3] == 4, "join() waits for every thread");
		g.spawn([&out] { out[0] = 10; });
		g.rethrow();
		check(out[0] == 10, "a thread spawned after a join is joined too");
	}
	{   // threads still running when their owner goes out of scope are joined before what they write is destroyed (the owner
		// is declared after it); the sanitizers report a write into freed or out-of-scope memory
		std::atomic<int> done{ 0 };
		for (int round = 0; round < 4; ++round) {
			std::unique_ptr<std::vector<int>> heap(new std::vector<int>(1 << 12, 0));
			int local[64] = {};
			SideThreads g;
			for (int t = 0; t < 3; ++t)
				g.spawn([&, t] {
					pause_ms(20);
					for (size_t i = t; i < heap->size(); i += 3) (*heap)[i] = (int)i;
					local[t] = t + 1;
					done.fetch_add(1);
				});
		}
		check(done.load() == 12, "every thread ran to its end before its owner went");
	}
	if (failures) return 1;
	printf("ok\n");
	return 0;
}
