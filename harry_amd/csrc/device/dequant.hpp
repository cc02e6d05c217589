// Rescaling of quantised values (structs/quant.h:98-112) and the dequantisation into a component's original type
// (quant.h:180-212), on the device.  Shared by k_requant (kernels.hip, in place), k_render_gather (render.hip, to f32),
// k_distortion_rows (distortion.hip) and k_quant_sweep (sweep.hip, every width in registers).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "codec_math.hpp"
#include "dev_types.hpp"
#include "fan.hpp"

namespace hry {
namespace dev {

// quant.h:103-107: val / from * to + val % from * to / from, in the type C++ evaluates it in (int for the 1- and 2-byte types).
// The products and the sum overflow that type for `ushort` at 16 bits (65 534 * 65 535 in int) and for `int` / `long` over most of
// their range; the reference's build wraps them and divides the wrapped product as a signed number.  A compiler that takes signed
// overflow for impossible divides it unsigned, so they are taken in the unsigned type and converted back.
template <typename T> __device__ __forceinline__ T rescale_int(T val, T from, T to)
{
	typedef decltype(val * to) P;
	typedef typename cm::word<sizeof(P)>::u U;
	const P v = val, f = from, t = to;
	const P whole = (P)((U)(v / f) * (U)t);
	const P part = (P)((U)(v % f) * (U)t) / f;
	return (T)(P)((U)whole + (U)part);
}

template <typename T> __device__ __forceinline__ T rescale_fp(T val, T from, T to) { return val / from * to; }   // quant.h:98-102 (every operation rounded on its own)

// q (c.src_bits quantisation bits) -> rescale(q, 2^bits - 1, extent) + min in c.dst_type; the raw bits of that value, in the low
// bytes of the word (what the original-width slot holds)
__device__ __forceinline__ uint64_t dequantise_bits(uint64_t q, const RequantComp &c)
{
	const int sl = (1 << (uint32_t)c.src_bits) - 1;
	switch (c.dst_type) {
	case 0: return cm::bits<uint32_t>(rescale_fp<float>((float)q, (float)sl, cm::bits<float>((uint32_t)c.scale)) + cm::bits<float>((uint32_t)c.mn));
	case 1: return cm::bits<uint64_t>(rescale_fp<double>((double)q, (double)sl, cm::bits<double>(c.scale)) + cm::bits<double>(c.mn));
	case 2: return rescale_int<uint64_t>(q, (uint64_t)sl, c.scale) + c.mn;
	case 3: return (uint64_t)rescale_int<int64_t>((int64_t)q, (int64_t)sl, (int64_t)c.scale) + c.mn;   // (the sum wraps)
	case 4: return (uint32_t)(rescale_int<uint32_t>((uint32_t)q, (uint32_t)sl, (uint32_t)c.scale) + (uint32_t)c.mn);
	case 5: return (uint32_t)rescale_int<int32_t>((int32_t)q, (int32_t)sl, (int32_t)c.scale) + (uint32_t)c.mn;
	case 6: return (uint16_t)(rescale_int<uint16_t>((uint16_t)q, (uint16_t)sl, (uint16_t)c.scale) + (uint16_t)c.mn);
	case 7: return (uint16_t)(rescale_int<int16_t>((int16_t)q, (int16_t)sl, (int16_t)c.scale) + (int16_t)c.mn);
	case 8: return (uint8_t)(rescale_int<uint8_t>((uint8_t)q, (uint8_t)sl, (uint8_t)c.scale) + (uint8_t)c.mn);
	case 9: return (uint8_t)(rescale_int<int8_t>((int8_t)q, (int8_t)sl, (int8_t)c.scale) + (int8_t)c.mn);
	default: return 0;
	}
}

// the raw bits of an unquantised component of type `type`, in the low bytes of the word
__device__ __forceinline__ uint64_t load_raw(const uint8_t *slot, int type)
{
	switch (type) {
	case 1: case 2: case 3: return ldg<uint64_t>(slot);
	case 6: case 7: return ldg<uint16_t>(slot);
	case 8: case 9: return ldg<uint8_t>(slot);
	default: return ldg<uint32_t>(slot);
	}
}

// the component's value after hry_requant(clear) -- quantised ones through dequantise_bits, the others as stored -- as a double
// (k_distortion_rows, k_distortion_normals)
__device__ __forceinline__ double component_f64(const uint8_t *slot, const RequantComp &c)
{
	uint64_t v;
	if (c.src_bits) {
		uint64_t q;
		switch (c.src_type) {   // storage type of the quantised value (quant.h:121-129)
		case 8: q = ldg<uint8_t>(slot); break;
		case 6: q = ldg<uint16_t>(slot); break;
		case 4: q = ldg<uint32_t>(slot); break;
		default: q = ldg<uint64_t>(slot); break;
		}
		v = dequantise_bits(q, c);
	} else v = load_raw(slot, c.dst_type);
	return cm::value_f64(v, c.dst_type);
}

// an unquantised value (raw: load_raw of c.src_type) -> its c.dst_bits quantisation bits (quant.h:131-166), before the store
// narrows them (stored_bits)
__device__ __forceinline__ uint64_t quantise_raw(uint64_t raw, const RequantComp &c)
{
	const int lv = (1 << (uint32_t)c.dst_bits) - 1;   // levels of the destination; evaluated in int like the reference (quant.h:135)
	switch (c.src_type) {
	case 0: return cm::quantise_f32(cm::bits<float>((uint32_t)raw), cm::bits<float>((uint32_t)c.mn), cm::bits<float>((uint32_t)c.scale), c.dst_bits);
	case 1: return (uint64_t)(rescale_fp<double>(cm::bits<double>(raw) - cm::bits<double>(c.mn), cm::bits<double>(c.scale), (double)lv) + 0.5);
	case 2: return rescale_int<uint64_t>(raw - c.mn, c.scale, (uint64_t)lv);
	case 3: return (uint64_t)rescale_int<int64_t>((int64_t)(raw - c.mn), (int64_t)c.scale, (int64_t)lv);   // (the distance to the minimum wraps)
	case 4: return rescale_int<uint32_t>((uint32_t)raw - (uint32_t)c.mn, (uint32_t)c.scale, (uint32_t)lv);
	case 5: return (uint64_t)rescale_int<int32_t>((int32_t)((uint32_t)raw - (uint32_t)c.mn), (int32_t)c.scale, (int32_t)lv);
	case 6: return rescale_int<uint16_t>((uint16_t)((uint16_t)raw - (uint16_t)c.mn), (uint16_t)c.scale, (uint16_t)lv);
	case 7: return (uint64_t)rescale_int<int16_t>((int16_t)((int16_t)(uint16_t)raw - (int16_t)c.mn), (int16_t)c.scale, (int16_t)lv);
	case 8: return rescale_int<uint8_t>((uint8_t)((uint8_t)raw - (uint8_t)c.mn), (uint8_t)c.scale, (uint8_t)lv);
	case 9: return (uint64_t)rescale_int<int8_t>((int8_t)((int8_t)(uint8_t)raw - (int8_t)c.mn), (int8_t)c.scale, (int8_t)lv);
	default: return 0;
	}
}
// what a slot keeps of q at `bits` quantisation bits: its storage type is u8 up to 8 bits, u16 up to 16, u32 above (mixing.h:101-108)
__device__ __forceinline__ uint64_t stored_bits(uint64_t q, int bits) { return bits <= 8 ? (uint8_t)q : bits <= 16 ? (uint16_t)q : (uint32_t)q; }

// what hry_requant to q bits followed by the -c dequantisation makes of the unquantised value raw, as a double (k_quant_sweep,
// k_normal_sweep).  T: the component's type at compile time, or -1: c's
template <int T> __device__ __forceinline__ double value_at(uint64_t raw, const RequantComp &c, int q)
{
	RequantComp k = c;
	if (T >= 0) { k.src_type = T; k.dst_type = T; }
	k.src_bits = 0; k.dst_bits = q;
	const uint64_t stored = stored_bits(quantise_raw(raw, k), q);
	k.src_bits = q; k.dst_bits = 0;
	return cm::value_f64(dequantise_bits(stored, k), k.dst_type);
}

}   // namespace dev
}   // namespace hry
