// The product's scalar attribute arithmetic (codec_math.hpp: fold_int / unfold_int through residual_bits / value_from_residual,
// parallelogram, the float pair) against the reference's answers in tests/golden/kat.json, for every compiler the product is
// built with.  Rows on stdin, one per line, as tests/test_host_cpu.py writes them from the delta_* and predict_* sections:
//   df raw pred enc dec            float residual, all four as bit patterns
//   du|ds bytes q raw pred enc dec unsigned / signed integer residual
//   pf v0 v1 v2 r                  float parallelogram, bit patterns
//   pu|ps bytes q v0 v1 v2 r       unsigned / signed integer parallelogram
// Built and run by tests/test_host_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "codec_math.hpp"

namespace cm = hry::cm;

template <typename T> static bool delta_ok(long long raw, long long pred, long long enc, long long dec, int q)
{
	typedef typename cm::word<sizeof(T)>::u U;
	const U e = cm::residual_bits<T>((T)raw, (T)pred, q);
	const T d = cm::value_from_residual<T>((U)enc, (T)pred, q);
	return e == (U)enc && d == (T)dec;
}
template <typename T> static bool predict_ok(long long v0, long long v1, long long v2, long long r, int q)
{
	return cm::parallelogram<T>((T)v0, (T)v1, (T)v2, q) == (T)r;
}

int main()
{
	char kind[8];
	unsigned long long checked = 0, bad = 0;
	while (scanf("%7s", kind) == 1) {
		long long a[7];
		const bool fp = kind[1] == 'f';
		const int n = fp ? 4 : 6;
		for (int i = 0; i < n; ++i) if (scanf("%lld", &a[i]) != 1) { printf("short row\n"); return 2; }
		bool ok = false;
		if (!strcmp(kind, "df")) {
			const float raw = cm::bits<float>((uint32_t)a[0]), pred = cm::bits<float>((uint32_t)a[1]);
			ok = cm::residual_bits<float>(raw, pred, 0) == (uint32_t)a[2]
			     && cm::bits<uint32_t>(cm::value_from_residual<float>((uint32_t)a[2], pred, 0)) == (uint32_t)a[3];
		} else if (!strcmp(kind, "pf")) {
			const float r = cm::parallelogram<float>(cm::bits<float>((uint32_t)a[0]), cm::bits<float>((uint32_t)a[1]), cm::bits<float>((uint32_t)a[2]), 0);
			ok = cm::bits<uint32_t>(r) == (uint32_t)a[3];
		} else {
			const bool sg = kind[1] == 's', delta = kind[0] == 'd';
			const int bytes = (int)a[0], q = (int)a[1];
			if (kind[1] != 'u' && !sg) { printf("unknown row %s\n", kind); return 2; }
			if (delta) {
				if (bytes == 1) ok = sg ? delta_ok<int8_t>(a[2], a[3], a[4], a[5], q) : delta_ok<uint8_t>(a[2], a[3], a[4], a[5], q);
				else if (bytes == 2) ok = sg ? delta_ok<int16_t>(a[2], a[3], a[4], a[5], q) : delta_ok<uint16_t>(a[2], a[3], a[4], a[5], q);
				else ok = sg ? delta_ok<int32_t>(a[2], a[3], a[4], a[5], q) : delta_ok<uint32_t>(a[2], a[3], a[4], a[5], q);
			} else {
				if (bytes == 1) ok = sg ? predict_ok<int8_t>(a[2], a[3], a[4], a[5], q) : predict_ok<uint8_t>(a[2], a[3], a[4], a[5], q);
				else if (bytes == 2) ok = sg ? predict_ok<int16_t>(a[2], a[3], a[4], a[5], q) : predict_ok<uint16_t>(a[2], a[3], a[4], a[5], q);
				else ok = sg ? predict_ok<int32_t>(a[2], a[3], a[4], a[5], q) : predict_ok<uint32_t>(a[2], a[3], a[4], a[5], q);
			}
		}
		++checked;
		if (!ok) { if (bad < 8) printf("BAD %s %lld %lld %lld %lld\n", kind, a[0], a[1], a[2], a[3]); ++bad; }
	}
	printf("%llu checked, %llu bad\n", checked, bad);
	return bad != 0 || checked == 0;
}
