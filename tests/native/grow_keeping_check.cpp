// grow_keeping of harry_amd/csrc/device/grow_keeping.hpp -- a working buffer that grows between the two stretches of a build and
// keeps the first stretch's pieces -- against the sized stand-in for the runtime (fake_hip_sized/), under AddressSanitizer / UBSan.
// Built and run by tests/test_grow_keeping_cpu.py.  Prints "ok" and exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../harry_amd/csrc/device/grow_keeping.hpp"

using namespace hry;
using fake_hip::calls;

static int failures = 0;
static void check(bool ok, const char *what)
{
	if (!ok) { fprintf(stderr, "FAILED: %s (calls so far: \"%s\")\n", what, calls.c_str()); ++failures; }
}
static void fill(DevBuf &b, size_t n, uint8_t seed) { for (size_t i = 0; i < n; ++i) b.as<uint8_t>()[i] = (uint8_t)(seed + 7 * i); }
static bool holds(const DevBuf &b, size_t n, uint8_t seed)
{
	for (size_t i = 0; i < n; ++i) if (b.as<uint8_t>()[i] != (uint8_t)(seed + 7 * i)) return false;
	return true;
}

int main()
{
	Stream stream;
	hipStream_t st = stream;   // (created here: the one handle that stays to the end)
	{   // room enough: nothing happens
		DevBuf b;
		b.ensure(1000);
		fill(b, 1000, 3);
		void *was = b.p;
		const size_t cap = b.cap;
		calls.clear();
		check(!grow_keeping(b, 1000, 1000, st) && !grow_keeping(b, cap, 64, st) && !grow_keeping(b, 0, 0, st), "a size that fits does not grow");
		check(calls.empty() && b.p == was && b.cap == cap && holds(b, 1000, 3), "... and touches nothing");
	}
	{   // it grows: the kept bytes move, one copy waited for, the old block goes once
		DevBuf b;
		b.ensure(1000);
		fill(b, b.cap, 5);
		void *was = b.p;
		const size_t cap = b.cap;
		calls.clear();
		check(grow_keeping(b, cap + 1, 600, st), "a larger size grows");
		check(calls == "mcSf", "one allocation, one copy, waited for, then the old block freed");
		check(fake_hip::last_copy == 600 && b.p != was && b.cap >= cap + 1 && holds(b, 600, 5), "the first `keep` bytes are where they were");
		fill(b, b.cap, 9);   // (all of the new block is the buffer's)
		const size_t cap2 = b.cap;
		calls.clear();
		check(grow_keeping(b, 10 * cap2, (size_t)1 << 30, st) && fake_hip::last_copy == cap2 && holds(b, cap2, 9), "no more is copied than the old block held");
		check(calls == "mcSf", "... in the same four calls");
		calls.clear();
		check(grow_keeping(b, 2 * b.cap, 0, st) && calls == "mf", "nothing to keep: no copy and no wait");
	}
	check(fake_hip::live.size() == 1, "every block is freed, the stream alone is left");
	{   // an empty buffer grows as ensure does
		DevBuf b;
		calls.clear();
		check(grow_keeping(b, 100, 50, st) && calls == "m" && b.p && b.cap >= 100, "an empty buffer has nothing to copy");
	}
	{   // the new block cannot be had: the buffer is as it was
		DevBuf b;
		b.ensure(500);
		fill(b, 500, 11);
		void *was = b.p;
		const size_t cap = b.cap;
		calls.clear();
		fake_hip::fail_in = 1;
		bool threw = false;
		try { grow_keeping(b, 10 * cap, 500, st); } catch (const Error &) { threw = true; }
		check(threw && calls.empty() && b.p == was && b.cap == cap && holds(b, 500, 11), "a failed allocation leaves the buffer and its bytes");
		check(grow_keeping(b, 10 * cap, 500, st) && holds(b, 500, 11), "... and the next call grows it");
	}
	check(fake_hip::live.size() == 1, "every block is freed in the end");
	if (failures) return 1;
	puts("ok");
	return 0;
}
