// The counting stand-in of ../../fake_hip, with device memory of the size asked for and the device copy: what
// harry_amd/csrc/device/grow_keeping.hpp calls beyond hip_handles.hpp.  A block is a real heap block of its size, so AddressSanitizer
// sees a copy that reads or writes past either end.  'c': a copy; fake_hip::last_copy: its bytes.
#pragma once
#define hipMalloc fake_hip_one_byte_malloc   // (the stand-in's blocks are one byte whatever is asked: replaced below)
#include "../../fake_hip/hip/hip_runtime.h"
#undef hipMalloc
#include <cstring>

enum hipMemcpyKind { hipMemcpyDeviceToDevice = 3 };
namespace fake_hip {
inline size_t last_copy = 0;
}
inline hipError_t hipMalloc(void **p, size_t n)
{
	fake_hip::last_malloc = n;
	if (fake_hip::fail_in && --fake_hip::fail_in == 0) return hipErrorOutOfMemory;
	*p = malloc(n ? n : 1);
	fake_hip::live.insert(*p);
	fake_hip::calls += 'm';
	return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
	if (kind != hipMemcpyDeviceToDevice || !fake_hip::live.count(s)) return hipErrorInvalidValue;
	memcpy(dst, src, n);
	fake_hip::last_copy = n;
	fake_hip::calls += 'c';
	return hipSuccess;
}
