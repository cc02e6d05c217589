// Owners of what the HIP runtime hands out: streams, events, device and pinned memory, registered host ranges.  Nothing else in
// the library creates or destroys one of these, a result handle's device memory included (tests/test_hip_handles_cpu.py).  Streams
// and events are created when they are first used; a creation that fails throws and leaves the owner empty, so the next use tries
// again.  Not thread-safe: whoever shares an owner with a side thread touches it (get()) before the thread starts.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/harry_amd.h"
#include "../host/mesh.hpp"

namespace hry {

inline void hip_check(hipError_t e, const char *what)
{
	if (e != hipSuccess) throw Error(HRY_E_NODEVICE, std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
#define HIP_OK(x) ::hry::hip_check((x), #x)

// a non-blocking stream; stands wherever a hipStream_t is expected.  Its work is waited for before it goes
struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
	~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
	void create(int priority) { hipStream_t n = nullptr; HIP_OK(hipStreamCreateWithPriority(&n, hipStreamNonBlocking, priority)); s = n; }   // (an empty owner: the context's main stream)
	hipStream_t get()
	{
		if (!s) { hipStream_t n = nullptr; HIP_OK(hipStreamCreateWithFlags(&n, hipStreamNonBlocking)); s = n; }
		return s;
	}
	operator hipStream_t() { return get(); }
	bool made() const { return s != nullptr; }
	void wait() const { if (s) (void)hipStreamSynchronize(s); }   // (a stream that was never used: nothing to wait for)
};

// an event; stands wherever a hipEvent_t is expected.  Event orders streams, TimedEvent can be asked for elapsed times as well
template <unsigned kFlags> struct EventWith {
	hipEvent_t e = nullptr;
	EventWith() = default;
	EventWith(EventWith &&o) noexcept : e(o.e) { o.e = nullptr; }
	~EventWith() { if (e) (void)hipEventDestroy(e); }
	hipEvent_t get()
	{
		if (!e) { hipEvent_t n = nullptr; HIP_OK(hipEventCreateWithFlags(&n, kFlags)); e = n; }
		return e;
	}
	operator hipEvent_t() { return get(); }
	bool made() const { return e != nullptr; }
};
typedef EventWith<hipEventDisableTiming> Event;
typedef EventWith<hipEventDefault> TimedEvent;

// a range of the caller's pageable memory made readable by the copy engines where it lies, for as long as the owner lives.  The
// runtime may refuse (pin() returns false, the error is cleared): the caller copies through memory of its own then
struct HostRegistration {
	void *p = nullptr;
	HostRegistration() = default;
	HostRegistration(const HostRegistration&) = delete;
	HostRegistration &operator=(const HostRegistration&) = delete;
	~HostRegistration() { release(); }
	bool pin(const void *q, size_t n)
	{
		release();
		if (hipHostRegister(const_cast<void*>(q), n, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return false; }
		p = const_cast<void*>(q);
		return true;
	}
	void release() { if (p) { (void)hipHostUnregister(p); p = nullptr; } }
};

struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf &operator=(const DevBuf&) = delete;
	~DevBuf() { if (p) (void)hipFree(p); }
	void ensure(size_t n)
	{
		if (n <= cap) return;
		if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
		size_t want = n + n / 8 + 256;
		HIP_OK(hipMalloc(&p, want));
		cap = want;
	}
	template <typename T> T *as() const { return (T*)p; }
};

// the one allocation a result handle owns (context.hpp: DeviceResult): exactly the bytes asked for -- it is sized once and kept as
// long as the caller keeps the handle, so DevBuf's slack for growth would never be used -- and freed on its own device, whichever
// device the thread that drops the handle has selected
struct DeviceBlock {
	int device = 0;
	void *p = nullptr;
	size_t bytes = 0;
	DeviceBlock() = default;
	DeviceBlock(const DeviceBlock&) = delete;
	DeviceBlock &operator=(const DeviceBlock&) = delete;
	~DeviceBlock() { if (p) { (void)hipSetDevice(device); (void)hipFree(p); } }
	void alloc(int dev, size_t n)   // (once; dev: the device the caller has selected)
	{
		if (p) throw Error(HRY_E_INTERNAL, "a device block is allocated once");
		void *q = nullptr;
		HIP_OK(hipMalloc(&q, n));
		device = dev; p = q; bytes = n;
	}
};

// one allocation in 256-byte aligned pieces: take(pointer, bytes) every piece while sizing, allocate `total` bytes, then bind(base)
// points every pointer taken at its piece of the block -- a piece is stated once, with the pointer it is for.  The pointers are
// written where they lay at take(): fields of the object the kernels get, not of a copy made in between.  reserve() / ptr() are
// the same step in two halves, for pieces found by index (OutputPlan, DedupPlan, VertexRows, a piece per list).  A piece of 0
// bytes takes one unit all the same, so no two pieces share an address (nobody depends on the smallest piece's size)
struct Carve {
	static constexpr size_t kAlign = 256;
	std::vector<size_t> at;
	std::vector<std::pair<void*, size_t>> taken;   // where a pointer lies, and its piece
	size_t total = 0;
	size_t reserve(size_t bytes) { at.push_back(total); total += (std::max<size_t>(bytes, 1) + kAlign - 1) & ~(kAlign - 1); return at.size() - 1; }
	template <typename T> T *ptr(void *base, size_t i) const { return (T*)((uint8_t*)base + at[i]); }
	template <typename T> void take(T *&pointer, size_t bytes) { taken.emplace_back((void*)&pointer, reserve(bytes)); }
	void bind(void *base) const
	{
		for (const auto &t : taken) { void *p = ptr<void>(base, t.second); memcpy(t.first, &p, sizeof p); }   // (every object pointer has void*'s representation)
	}
};

// pinned host memory, grow-only (persistent across calls: fresh pinned or pageable blocks cost a page fault per 4 KiB)
struct PinBuf {
	void *p = nullptr;
	size_t cap = 0;
	PinBuf() = default;
	PinBuf(const PinBuf&) = delete;
	PinBuf &operator=(const PinBuf&) = delete;
	~PinBuf() { if (p) (void)hipHostFree(p); }
	void ensure(size_t n)
	{
		if (n <= cap) return;
		if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
		size_t want = n + n / 8 + 4096;
		HIP_OK(hipHostMalloc(&p, want, hipHostMallocDefault));
		cap = want;
	}
	template <typename T> T *as() const { return (T*)p; }
};

}   // namespace hry
