// A working buffer that has to grow between the two stretches of a build while the first stretch's pieces are still needed
// (user: bvh.cpp, hry_intersections_build; result_build.hpp includes this).  It rests on hip_handles.hpp alone, so that
// tests/native/grow_keeping_check.cpp holds it against a stand-in for the runtime under the sanitizers.
#pragma once
#include "hip_handles.hpp"

namespace hry {

// b.ensure(n) for a buffer whose first `keep` bytes are still needed: where it has to grow, the new block takes them over (no more
// than the old block held) by a device copy on st, waited for, before the old block goes.  true: it grew.  Where the new block
// cannot be had, b is as it was
inline bool grow_keeping(DevBuf &b, size_t n, size_t keep, hipStream_t st)
{
	if (n <= b.cap) return false;
	DevBuf larger;
	larger.ensure(n);
	if (b.p && keep) {
		HIP_OK(hipMemcpyAsync(larger.p, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, st));
		HIP_OK(hipStreamSynchronize(st));
	}
	std::swap(b.p, larger.p);
	std::swap(b.cap, larger.cap);
	return true;   // (the old block is freed with `larger`)
}

}   // namespace hry
