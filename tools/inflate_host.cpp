// inflate_host.cpp -- the decode logic of csrc/inflate.h on the CPU, with the host compiler alone: the exact functions
// the kernels of csrc/inflate.hip run, one "lane" wide.  tests/test_inflate_host.py compares it with the definition,
// tests/inflate_ref.py; a build with -fsanitize=address,undefined checks the same logic for reads out of range.
//
//   c++ -std=c++17 -O1 -o inflate_host tools/inflate_host.cpp
//   inflate_host corpus.bin
//
// The file holds records: uint64 zbytes, uint64 n, uint64 entries (little endian), the stream's bytes, then per entry
// header_bit and token_bit (uint64 each).  Per record one line: status bad_chunk adler32 literals matches matched_bytes.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../cuttlefish_amd/csrc/inflate.h"

static bool read_exact(FILE* f, void* p, size_t n)
{
	return n == 0 || fread(p, 1, n, f) == n;
}

struct Verdict {
	uint32_t status = 0, bad_chunk = 0, adler = 0;
	uint64_t literals = 0, matches = 0, matched = 0;
};

static Verdict run(const std::vector<uint8_t>& z, uint64_t n, const std::vector<cfinf_entry>& index)
{
	Verdict v;
	const uint64_t C = (n + CFINF_CHUNK - 1u)/CFINF_CHUNK;
	std::unique_ptr<CfinfWork> w(new CfinfWork);
	std::vector<uint32_t> S(n);
	for (uint64_t c = 0; c < (C ? C : 1u); ++c) {
		const uint32_t want = C ? (uint32_t)(n - c*CFINF_CHUNK < CFINF_CHUNK ? n - c*CFINF_CHUNK : CFINF_CHUNK) : 0u;
		const uint32_t e = cfinf_chunk(*w, z.data(), z.size(), index.data(), C, c, want, 0u, 1u);
		if (e != CFINF_OK) {
			v.status = e;
			v.bad_chunk = (uint32_t)c;
			return v;
		}
		v.literals += w->literals;
		v.matches += w->matches;
		v.matched += w->matched;
		// the expansion the way the kernel's lanes do it: 64 positions from the token that covers the first
		const uint64_t base = c*CFINF_CHUNK;
		for (uint32_t lane = 0; lane < 64u && 64u*lane < want; ++lane) {
			uint32_t p0 = w->cover[lane];
			uint32_t t = w->S[CFINF_PAD(p0)];
			uint32_t end = p0 + ((t & CFINF_MATCH) ? (t & 0xFFu) + 3u : 1u);
			for (uint32_t i = 64u*lane; i < 64u*lane + 64u && i < want; ++i) {
				if (i == end) {
					p0 = i;
					t = w->S[CFINF_PAD(i)];
					end = p0 + ((t & CFINF_MATCH) ? (t & 0xFFu) + 3u : 1u);
				}
				S[base + i] = cfinf_expand(t, p0, i, base);
			}
		}
	}
	// pointers are strictly below their position: one ascending pass resolves them
	uint32_t a = 1u, b = 0u;
	for (uint64_t i = 0; i < n; ++i) {
		uint32_t s = S[i];
		if (s & CFINF_PTR) {
			const uint64_t q = s & ~CFINF_PTR;
			s = q < i ? S[q] : 0u;
			S[i] = s;
		}
		a = (a + (s & 0xFFu)) % 65521u;
		b = (b + a) % 65521u;
	}
	v.adler = (b << 16) | a;
	const uint8_t* t = z.data() + z.size() - 4;
	const uint32_t stored = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
	if (stored != v.adler) {
		v.status = CFINF_E_CHECKSUM;
		v.bad_chunk = (uint32_t)(C ? C - 1u : 0u);
	}
	return v;
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: inflate_host corpus.bin\n");
		return 2;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	uint64_t head[3];
	while (fread(head, 8, 3, f) == 3) {
		if (head[0] > ((uint64_t)1 << 32) || head[1] > ((uint64_t)1 << 31) || head[2] > ((uint64_t)1 << 20)) {
			fprintf(stderr, "bad record\n");
			return 2;
		}
		std::vector<uint8_t> z(head[0]);
		std::vector<cfinf_entry> index(head[2]);
		if (!read_exact(f, z.data(), z.size()) || !read_exact(f, index.data(), index.size()*sizeof(cfinf_entry))) {
			fprintf(stderr, "truncated record\n");
			return 2;
		}
		if (index.size() < (head[1] + CFINF_CHUNK - 1u)/CFINF_CHUNK) {
			fprintf(stderr, "too few entries\n");
			return 2;
		}
		const Verdict v = run(z, head[1], index);
		const bool ok = v.status == 0;
		printf("%u %u %u %llu %llu %llu\n", v.status, v.bad_chunk, ok ? v.adler : 0u, ok ? (unsigned long long)v.literals : 0ull,
			ok ? (unsigned long long)v.matches : 0ull, ok ? (unsigned long long)v.matched : 0ull);
	}
	fclose(f);
	return 0;
}
