// A counting stand-in for the HIP runtime: the calls harry_amd/csrc/device/hip_handles.hpp makes, and nothing else.  Every call
// appends a letter to fake_hip::calls; handles are real heap blocks, so AddressSanitizer sees a leak or a second destroy as well.
// fake_hip::fail_in = n makes the n-th creation from now on (stream, event, allocation or registration) fail.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <set>
#include <string>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct fake_hip_stream *hipStream_t;
typedef struct fake_hip_event *hipEvent_t;
enum { hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipHostRegisterPortable = 1 };

namespace fake_hip {
inline std::string calls;          // s S x: stream created, synchronised, destroyed; e t y: event created (untimed, timed), destroyed;
                                   // m f: device memory; p q: pinned memory; r u: host range registered, unregistered; g: error cleared;
                                   // d: device selected
inline int fail_in = 0, last_priority = 0, device = 0;
inline size_t last_malloc = 0;     // bytes asked of the last hipMalloc
inline std::set<void*> live, ranges;
inline int count(char c) { return (int)std::count(calls.begin(), calls.end(), c); }
inline hipError_t make(void **out, char c)
{
	if (fail_in && --fail_in == 0) return hipErrorOutOfMemory;
	*out = malloc(1);
	live.insert(*out);
	calls += c;
	return hipSuccess;
}
inline hipError_t drop(void *h, char c)
{
	if (!live.erase(h)) return hipErrorInvalidValue;   // (not a handle, or destroyed before)
	free(h);
	calls += c;
	return hipSuccess;
}
}

inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake failure"; }
inline hipError_t hipGetLastError() { fake_hip::calls += 'g'; return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { return flags == hipStreamNonBlocking ? fake_hip::make((void**)s, 's') : hipErrorInvalidValue; }
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority) { fake_hip::last_priority = priority; return hipStreamCreateWithFlags(s, flags); }
inline hipError_t hipStreamSynchronize(hipStream_t s) { if (!fake_hip::live.count(s)) return hipErrorInvalidValue; fake_hip::calls += 'S'; return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::drop(s, 'x'); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { return fake_hip::make((void**)e, flags == hipEventDisableTiming ? 'e' : 't'); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::drop(e, 'y'); }
inline hipError_t hipSetDevice(int d) { fake_hip::device = d; fake_hip::calls += 'd'; return hipSuccess; }
inline hipError_t hipMalloc(void **p, size_t n) { fake_hip::last_malloc = n; return fake_hip::make(p, 'm'); }
inline hipError_t hipFree(void *p) { return fake_hip::drop(p, 'f'); }
inline hipError_t hipHostMalloc(void **p, size_t, unsigned) { return fake_hip::make(p, 'p'); }
inline hipError_t hipHostFree(void *p) { return fake_hip::drop(p, 'q'); }
inline hipError_t hipHostRegister(void *p, size_t, unsigned)
{
	if ((fake_hip::fail_in && --fake_hip::fail_in == 0) || !fake_hip::ranges.insert(p).second) return hipErrorInvalidValue;
	fake_hip::calls += 'r';
	return hipSuccess;
}
inline hipError_t hipHostUnregister(void *p)
{
	if (!fake_hip::ranges.erase(p)) { fake_hip::calls += '!'; return hipErrorInvalidValue; }   // (never registered: '!' fails the check)
	fake_hip::calls += 'u';
	return hipSuccess;
}
