// Numbering maps of an encode (include/harry_amd.h: hry_order_take): which decoded element every source element becomes, the
// inverses, and the kernel that moves a caller's rows through a map.  Integer work only, wave64, a lane per output word.
//   k_order_vertex   vertex[org[order_v[j]]] = j, vertex_inv[j] = the vertex                  (what k_rank computes, with its inverse)
//   k_order_face     face[face_of(order_f[j])] = j, face_inv[j] = the face, and the face's degree in coding order (mixed degrees)
//   k_scan_*         (scan.hip: launch_excl_scan, from order.cpp) exclusive scan of those degrees: where every decoded face begins.  Uniform degree: j * degree
//   k_order_corner   the decoder makes the half-edge a face is entered through the face's first (cbm/decoder.h:75-77 for a
//                    component's first face, :162-164 for the rest, where e0 is the twin of the gate) and keeps the cyclic order: the
//                    corner k places behind order_f[j] round source face f becomes decoded half-edge doff[j] + k
//   k_order_records  general bindings: list[d_idx[j]] = j over the records in creation order, and the inverse
//   k_order_rows     dst row i = src row map[i], zero bytes where the map says HRY_NO_ELEMENT: a lane per 16 bytes of dst where
//                    pointers, strides and row width are multiples of 16, per 4-byte word where multiples of 4, per byte otherwise
// Every table is pre-filled with 0xFF; the maps are injective on coded elements, so no two lanes write one slot.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "fan.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

__global__ __launch_bounds__(256) void k_order_vertex(const uint32_t *order_v, uint32_t n, const uint32_t *org, uint32_t nv, uint32_t *vertex, uint32_t *vertex_inv)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const uint32_t v = org[order_v[j]];
	if (v >= nv) return;
	vertex[v] = j;
	vertex_inv[j] = v;
}

__global__ __launch_bounds__(256) void k_order_face(ConnView cv, const uint32_t *order_f, uint32_t n, uint32_t *face, uint32_t *face_inv, uint32_t *deg)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const uint32_t e0 = order_f[j];
	if (e0 >= cv.ne) { if (deg) deg[j] = 0; return; }
	const uint32_t f = cv.eface ? cv.eface[e0] : e0 / cv.udeg;
	face[f] = j;
	face_inv[j] = f;
	if (deg) deg[j] = cv.foff[f + 1] - cv.foff[f];
}

// doff: first decoded half-edge of every coded face (mixed degrees), nullptr: j * udeg
__global__ __launch_bounds__(256) void k_order_corner(ConnView cv, const uint32_t *order_f, const uint32_t *face, const uint32_t *doff, uint32_t *corner, uint32_t *corner_inv)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= cv.ne) return;
	uint32_t f, d;
	if (cv.eface) { f = cv.eface[c]; d = cv.foff[f + 1] - cv.foff[f]; }
	else { f = c / cv.udeg; d = cv.udeg; }
	const uint32_t j = face[f];
	if (j == kNoRank) return;
	const uint32_t e0 = order_f[j];
	const uint32_t k = c >= e0 ? c - e0 : c + d - e0;
	const uint32_t to = (doff ? doff[j] : j * cv.udeg) + k;
	if (to >= cv.ne) return;
	corner[c] = to;
	corner_inv[to] = c;
}

__global__ __launch_bounds__(256) void k_order_records(const uint32_t *d_idx, uint32_t nd, uint32_t count, uint32_t *list, uint32_t *list_inv)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= nd || j >= count) return;
	const uint32_t r = d_idx[j];
	if (r >= count) return;
	list[r] = j;
	list_inv[j] = r;
}

// T: the unit a lane moves (Quad: 16 bytes, uint32_t: the word path, uint8_t: the byte path); upr units per row; strides in bytes
struct alignas(16) Quad { uint32_t x, y, z, w; };
template <typename T>
__global__ __launch_bounds__(256) void k_order_rows(const uint32_t *map, uint64_t rows, const uint8_t *src, uint64_t src_stride, uint8_t *dst, uint64_t dst_stride, uint32_t upr, uint64_t total)
{
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= total) return;
	uint64_t row;
	uint32_t u;
	if (total <= 0xffffffffull) { const uint32_t g32 = (uint32_t)g; row = g32 / upr; u = g32 - (uint32_t)row * upr; }
	else { row = g / upr; u = (uint32_t)(g - row * upr); }
	const uint32_t from = map[row];
	T v = T{};
	if (from != kNoRank && from < rows) v = *(const T*)(src + (uint64_t)from * src_stride + (uint64_t)u * sizeof(T));
	*(T*)(dst + row * dst_stride + (uint64_t)u * sizeof(T)) = v;
}

void launch_order_vertex(hipStream_t st, const uint32_t *order_v, uint32_t n, const uint32_t *org, uint32_t nv, uint32_t *vertex, uint32_t *vertex_inv)
{
	if (n) hipLaunchKernelGGL(k_order_vertex, dim3(blocks_for(n, 256)), dim3(256), 0, st, order_v, n, org, nv, vertex, vertex_inv);
}
void launch_order_face(hipStream_t st, const ConnView &cv, const uint32_t *order_f, uint32_t n, uint32_t *face, uint32_t *face_inv, uint32_t *deg)
{
	if (n) hipLaunchKernelGGL(k_order_face, dim3(blocks_for(n, 256)), dim3(256), 0, st, cv, order_f, n, face, face_inv, deg);
}
void launch_order_corner(hipStream_t st, const ConnView &cv, const uint32_t *order_f, const uint32_t *face, const uint32_t *doff, uint32_t *corner, uint32_t *corner_inv)
{
	if (cv.ne) hipLaunchKernelGGL(k_order_corner, dim3(blocks_for(cv.ne, 256)), dim3(256), 0, st, cv, order_f, face, doff, corner, corner_inv);
}
void launch_order_records(hipStream_t st, const uint32_t *d_idx, uint32_t nd, uint32_t count, uint32_t *list, uint32_t *list_inv)
{
	if (nd) hipLaunchKernelGGL(k_order_records, dim3(blocks_for(nd, 256)), dim3(256), 0, st, d_idx, nd, count, list, list_inv);
}
bool launch_order_rows(hipStream_t st, const uint32_t *map, uint64_t rows, const void *src, uint64_t src_stride, void *dst, uint64_t dst_stride, uint64_t row_bytes)
{
	if (!rows) return true;
	const uint64_t all = (uintptr_t)src | (uintptr_t)dst | src_stride | dst_stride | row_bytes;
	const unsigned unit = (all & 15) == 0 ? 16 : (all & 3) == 0 ? 4 : 1;   // the widest unit that pointers, strides and row width are multiples of
	const uint64_t upr = row_bytes / unit;
	if (upr > 0xffffffffull || rows > (0x7fffffffull * 256) / upr) return false;   // (more lanes than one launch has)
	const uint64_t total = rows * upr;
	const dim3 grid(blocks_for(total, 256)), block(256);
	const uint8_t *s8 = (const uint8_t*)src;
	uint8_t *d8 = (uint8_t*)dst;
	if (unit == 16) hipLaunchKernelGGL(k_order_rows<Quad>, grid, block, 0, st, map, rows, s8, src_stride, d8, dst_stride, (uint32_t)upr, total);
	else if (unit == 4) hipLaunchKernelGGL(k_order_rows<uint32_t>, grid, block, 0, st, map, rows, s8, src_stride, d8, dst_stride, (uint32_t)upr, total);
	else hipLaunchKernelGGL(k_order_rows<uint8_t>, grid, block, 0, st, map, rows, s8, src_stride, d8, dst_stride, (uint32_t)upr, total);
	return true;
}

}   // namespace dev
}   // namespace hry
