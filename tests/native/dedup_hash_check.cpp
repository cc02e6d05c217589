// Prints what harry_amd/csrc/device/dedup_hash.hpp computes, for tests/test_dedup_cpu.py to compare with tests/dedup_ref.py.
// Includes nothing of the project but that header.  Standard input, one key per line:
//   w <hex digits>         a record of that many bytes / 2 (WeldKey); "w -" is the empty record
//   e <lo> <hi>            EdgeKey
//   s <shell> <vertex>     ShellVertexKey
//   c <vertex> <root>      CreaseKey
//   u <parts> <part> ...   UnweldKey: org, then one part per corner-target list
// Standard output: the hash of every key, decimal, one per line.  Exit status 1 on a line it cannot read.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dedup_hash.hpp"

static int hex_of(char c)
{
	if (c >= '0' && c <= '9') return c - '0';
	if (c >= 'a' && c <= 'f') return c - 'a' + 10;
	return -1;
}

int main()
{
	using namespace hry::dh;
	std::vector<char> line(1 << 16);
	std::vector<uint8_t> rec;
	while (fgets(line.data(), (int)line.size(), stdin)) {
		char *p = line.data();
		const char form = *p++;
		if (form == '\n' || form == 0) continue;
		uint32_t h = 0;
		if (form == 'w') {
			while (*p == ' ') ++p;
			rec.clear();
			if (*p != '-')
				for (; hex_of(p[0]) >= 0 && hex_of(p[1]) >= 0; p += 2) rec.push_back((uint8_t)(hex_of(p[0]) * 16 + hex_of(p[1])));
			else ++p;
			if (*p != '\n' && *p != 0) return 1;
			h = hash_bytes(rec.data(), (uint32_t)rec.size());
		} else if (form == 'e' || form == 's' || form == 'c') {
			char *q;
			const uint32_t a = (uint32_t)strtoul(p, &q, 10);
			if (q == p) return 1;
			p = q;
			const uint32_t b = (uint32_t)strtoul(p, &q, 10);
			if (q == p) return 1;
			h = form == 'e' ? hash_edge(a, b) : form == 's' ? hash_shell_vertex(a, b) : hash_crease(a, b);
		} else if (form == 'u') {
			char *q;
			const unsigned long parts = strtoul(p, &q, 10);
			if (q == p) return 1;
			p = q;
			h = hash_parts_start();
			for (unsigned long i = 0; i < parts; ++i) {
				const uint32_t part = (uint32_t)strtoul(p, &q, 10);
				if (q == p) return 1;
				p = q;
				h = hash_parts_step(h, part);
			}
		} else return 1;
		printf("%u\n", h);
	}
	return 0;
}
