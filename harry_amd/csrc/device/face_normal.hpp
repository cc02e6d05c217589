// A face's normal from its corners' positions, one corner at a time, and the chord between two unit normals: the arithmetic of
// the normal deviation (include/harry_amd.h: hry_normal_error; kernels: normal_sweep.hip).  N_f is the sum of the fan triangles'
// cross products relative to corner 0 -- the contract of hry_render_build_ex's face normals (k_nrm_faces, normals.hip, keeps its own
// float-row form of it) -- over "how a corner's position is obtained": the caller feeds fan_step the corners in order, from
// whatever it reads them.  A kernel that follows several versions of one face (one per quantisation width) keeps one FanSum each
// and nothing per corner.  Every operation is an individually rounded IEEE double operation in the written order
// (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 sub3(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross3(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double length3(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ bool usable_length(double len) { return len > 0.0 && len < __builtin_inf(); }   // (false for NaN)

// corner 0, the previous corner relative to it, and the sum so far (zero until the third corner)
struct FanSum { D3 p0, b, s; };
__device__ __forceinline__ void fan_clear(FanSum &f) { f.p0 = f.b = f.s = D3{ 0.0, 0.0, 0.0 }; }
// corner i (0, 1, 2, ... in the face's order) at position p
__device__ __forceinline__ void fan_step(FanSum &f, const D3 &p, uint32_t i)
{
	if (i == 0) { f.p0 = p; return; }
	const D3 a = f.b;
	f.b = sub3(p, f.p0);
	if (i == 1) return;
	const D3 t = cross3(a, f.b);
	if (i == 2) f.s = t;
	else { f.s.x += t.x; f.s.y += t.y; f.s.z += t.z; }   // polygons: the further fan triangles, in order
}
// n = N / |N|, one division per component; false: the face has no normal (|N| is 0 or not finite)
__device__ __forceinline__ bool unit_normal(const D3 &N, D3 &n)
{
	const double len = length3(N);
	if (!usable_length(len)) return false;
	n = D3{ N.x / len, N.y / len, N.z / len };
	return true;
}
// c2 = |n_y - n_x|^2 as (d.x*d.x + d.y*d.y) + d.z*d.z; the chord is sqrt(c2) = 2 sin(theta / 2)
__device__ __forceinline__ double chord_sq(const D3 &nx, const D3 &ny)
{
	const D3 d = sub3(ny, nx);
	return (d.x * d.x + d.y * d.y) + d.z * d.z;
}

}   // namespace dev
}   // namespace hry
