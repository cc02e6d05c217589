// The contract of harry_amd/csrc/device/hip_handles.hpp, against a counting stand-in for the runtime (fake_hip/), under
// AddressSanitizer / UBSan.  These are the paths a device error takes: no test provokes one on a device.
// Built and run by tests/test_hip_handles_cpu.py.  Prints "ok" and exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <deque>
#include <utility>
#include <vector>

#include "../../harry_amd/csrc/device/hip_handles.hpp"

using namespace hry;
using fake_hip::calls;
using fake_hip::count;

static int failures = 0;
static void check(bool ok, const char *what)
{
	if (!ok) { fprintf(stderr, "FAILED: %s (calls so far: \"%s\")\n", what, calls.c_str()); ++failures; }
}
template <typename F> static bool throws_error(F &&f)
{
	try { f(); } catch (const Error &e) { return e.code == HRY_E_NODEVICE; }
	return false;
}
// what decode_streams_conn_first used to build behind one guard: a stream, two ordering events, two more streams, three events
struct Group { Stream first; Event order[2]; Stream more[2]; Event done[3]; };
static void use(hipStream_t) {}
static void use(hipEvent_t) {}

int main()
{
	{   // nothing is created until first use; one creation however often it is used; one destroy; a stream is waited for first
		{
			Stream s; Event e; TimedEvent t; Group g;
			check(calls.empty() && !s.made() && !e.made() && !t.made(), "nothing is created until first use");
			s.wait();
			check(calls.empty(), "waiting for a stream that was never used does nothing");
			use(s); use(s); use(e); use(e); use(t); use(t);
			check(calls == "set" && s.made() && e.made() && t.made(), "each handle is created once, events with their own flag");
			hipStream_t raw = s;
			check(raw == s.s && raw == s.get(), "the owner stands for its handle");
		}
		check(calls == "setyySx", "each handle is destroyed once, a stream after it was synchronised");
	}
	calls.clear();
	{   // the main stream: created at once, with its priority
		Stream s;
		s.create(-3);
		use(s);
		check(calls == "s" && fake_hip::last_priority == -3, "create(priority) makes the stream, a later use does not make another");
	}
	check(calls == "sSx", "the stream's destructor synchronises before it destroys");
	calls.clear();
	{   // a moved-from handle destroys nothing; containers of owners move them
		{
			Event a;
			use(a);
			Event b(std::move(a));
			check(!a.made() && b.made(), "a move empties its source");
			Stream s;
			use(s);
			Stream s2(std::move(s));
			check(!s.made() && s2.made(), "a move empties its source (stream)");
		}
		check(calls == "esSxy", "a moved-from handle destroys nothing");
		calls.clear();
		{
			std::vector<Event> v;
			for (int i = 0; i < 9; ++i) { Event e; if (i % 3) use(e); v.push_back(std::move(e)); }   // (grows several times)
			std::deque<TimedEvent> d;
			for (int i = 0; i < 5; ++i) { d.emplace_back(); use(d.back()); }
			d.pop_front();
			check(count('e') == 6 && count('t') == 5 && count('y') == 1 && v[0].made() == false && v[1].made(), "owners in containers: created where used, destroyed with their element");
			v.resize(12);
			check(count('e') == 6, "a resize creates nothing");
		}
		check(count('y') == 11, "a container destroys exactly what was created");
	}
	calls.clear();
	{   // a failed creation throws Error, leaves the owner empty, and the next use tries again
		{
			Stream s; Event e;
			fake_hip::fail_in = 1;
			check(throws_error([&] { use(s); }) && !s.made(), "a failed stream creation throws and leaves the owner empty");
			fake_hip::fail_in = 1;
			check(throws_error([&] { use(e); }) && !e.made(), "a failed event creation throws and leaves the owner empty");
			check(calls.empty(), "nothing was created");
			use(s); use(e);
			check(calls == "se" && s.made() && e.made(), "a later use retries the creation");
			Stream p;
			fake_hip::fail_in = 1;
			check(throws_error([&] { p.create(0); }) && !p.made(), "a failed create(priority) leaves the owner empty");
		}
		check(calls == "seySx", "what the retries created is destroyed once");
	}
	calls.clear();
	{   // a group in which one creation fails destroys exactly what was created -- and is whole after the next use
		{
			Group g;
			fake_hip::fail_in = 4;   // first, order[0], order[1] succeed; more[0] fails
			check(throws_error([&] { use(g.first); for (Event &e : g.order) use(e); for (Stream &s : g.more) use(s); for (Event &e : g.done) use(e); }), "the failing creation of a group throws");
			check(calls == "see" && g.first.made() && g.order[1].made() && !g.more[0].made() && !g.more[1].made() && !g.done[0].made(), "the group holds what was created before the failure");
			use(g.more[0]);
			check(calls == "sees", "the handle whose creation failed is created by its next use: no half-built group for good");
		}
		check(count('x') == 2 && count('S') == 2 && count('y') == 2, "a group destroys exactly those that were created");
	}
	calls.clear();
	{   // registered host ranges
		int a[4], b[4], c[4];
		{
			HostRegistration r[3];
			check(r[0].pin(a, sizeof a) && r[0].p == a, "a registration is kept");
			fake_hip::fail_in = 1;
			check(!r[1].pin(b, sizeof b) && r[1].p == nullptr, "a refused registration is a soft failure");
			check(calls == "rg", "... whose error is cleared");
			check(r[2].pin(c, sizeof c), "a registration is kept");
			r[2].release(); r[2].release();
			check(calls == "rgru", "release() unregisters once");
		}
		check(calls == "rgruu" && fake_hip::ranges.empty(), "the owner unregisters only what it registered");
	}
	calls.clear();
	{   // device and pinned memory: grow-only, the old block freed first, everything freed at the end
		{
			DevBuf d; PinBuf p;
			d.ensure(0); p.ensure(0);
			check(calls.empty(), "no memory until some is asked for");
			d.ensure(100); d.ensure(50); p.ensure(100); p.ensure(100);
			check(calls == "mp" && d.cap >= 100 && p.cap >= 100, "one block each");
			d.ensure(d.cap + 1); p.ensure(p.cap + 1);
			check(calls == "mpfmqp", "growing frees the old block first");
			fake_hip::fail_in = 1;
			check(throws_error([&] { d.ensure(d.cap + 1); }) && d.p == nullptr && d.cap == 0, "a failed allocation leaves the buffer empty");
		}
		check(count('m') == count('f') && count('p') == count('q'), "every block is freed");
	}
	calls.clear();
	{   // a result's block: nothing until alloc, exactly the bytes asked for, freed once on its own device
		{
			DeviceBlock b;
			check(calls.empty() && b.p == nullptr && b.bytes == 0, "no block until alloc");
			b.alloc(3, 1000);
			check(calls == "m" && fake_hip::last_malloc == 1000 && b.p && b.bytes == 1000 && b.device == 3, "alloc asks for exactly n bytes");
			fake_hip::device = 0;
		}
		check(calls == "mdf" && fake_hip::device == 3, "the block's device is selected, then the block is freed: once each");
		calls.clear();
		{
			DeviceBlock b;
			fake_hip::fail_in = 1;
			check(throws_error([&] { b.alloc(1, 64); }) && b.p == nullptr && b.bytes == 0, "a failed alloc throws and leaves the owner empty");
		}
		check(calls.empty(), "an empty block selects no device and frees nothing");
	}
	{   // the carver: 256-byte aligned pieces in order, a piece of its own even for 0 bytes
		const size_t sizes[] = { 0, 1, 255, 256, 257, 0, 0, 1000, 256, 0 };
		Carve c;
		check(c.total == 0, "an empty carve has no bytes");
		std::vector<size_t> piece;
		for (size_t n : sizes) piece.push_back(c.reserve(n));
		alignas(256) static uint8_t base[16 * 256];
		bool ok = c.total <= sizeof base;
		for (size_t i = 0; i < piece.size() && ok; ++i) {
			const size_t at = (size_t)(c.ptr<uint8_t>(base, piece[i]) - base), end = at + sizes[i];
			const size_t next = i + 1 < piece.size() ? (size_t)(c.ptr<uint8_t>(base, piece[i + 1]) - base) : c.total;
			ok = piece[i] == i && at % 256 == 0 && end <= next && at < next && (uintptr_t)c.ptr<uint32_t>(base, piece[i]) % 256 == 0;
		}
		check(ok, "every piece is 256-byte aligned, begins at or after the end of the one before, and has an address of its own");
		check(c.total % 256 == 0 && c.total == (size_t)(c.ptr<uint8_t>(base, piece.back()) - base) + 256, "total is the end of the last piece");
		check(c.total == 256 * (1 + 1 + 1 + 1 + 2 + 1 + 1 + 4 + 1 + 1), "an empty piece takes one unit, the others their size rounded up");

		// take / bind: the same pieces in one statement each -- the addresses reserve / ptr hand out for the same sequence, whatever
		// the pointers' types, reserve()d pieces in between included; nothing is written before bind()
		struct Work { uint32_t *a = nullptr; double *b = nullptr; const uint8_t *k = nullptr; float *f = nullptr; unsigned long long *q = nullptr; uint32_t *z[5] = {}; } w;
		Carve t;
		t.take(w.a, sizes[0]); t.take(w.b, sizes[1]); t.take(w.k, sizes[2]); t.take(w.f, sizes[3]); t.take(w.q, sizes[4]);
		const size_t between = t.reserve(sizes[5]);   // (a piece found by index, as DedupPlan's)
		for (size_t i = 6; i < 10; ++i) t.take(w.z[i - 6], sizes[i]);
		check(t.total == c.total && t.at == c.at && between == 5, "take lays the pieces out as reserve does");
		check(!w.a && !w.b && !w.k && !w.f && !w.q && !w.z[0] && !w.z[3], "take writes no pointer");
		t.bind(base);
		const void *got[] = { w.a, w.b, w.k, w.f, w.q, t.ptr<void>(base, between), w.z[0], w.z[1], w.z[2], w.z[3] };
		bool same = true, apart = true;
		for (size_t i = 0; i < 10; ++i) {
			same = same && got[i] == c.ptr<void>(base, piece[i]);
			for (size_t j = 0; j < i; ++j) apart = apart && got[i] != got[j];
		}
		check(same, "bind hands out the addresses of reserve / ptr for the same sequence");
		check(apart && w.z[4] == nullptr, "no two pieces share an address, and a pointer that was not taken is left alone");
		alignas(256) static uint8_t other[16 * 256];
		t.bind(other);
		check((const uint8_t*)w.a == other && (const uint8_t*)w.z[3] == other + (c.ptr<uint8_t>(base, piece[9]) - base), "a second bind moves every pointer to the new block");
		Carve none;
		none.bind(base);
		check(none.total == 0, "an empty carve binds nothing");
	}
	check(fake_hip::live.empty() && fake_hip::ranges.empty() && calls.find('!') == std::string::npos, "the counts balance at exit");
	if (failures) return 1;
	printf("ok\n");
	return 0;
}
