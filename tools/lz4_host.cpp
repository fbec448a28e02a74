// lz4_host.cpp -- the decode logic of csrc/lz4.h on the CPU, with the host compiler alone: the exact functions the
// kernels of csrc/lz4.hip call for the frame header, the block chain and every sequence.  tests/test_lz4_host.py compares
// it with the definition, tests/lz4_ref.py; a build with -fsanitize=address,undefined checks the same logic for reads
// and writes out of range (the frame and the output live in heap blocks of their exact sizes).
//
//   c++ -std=c++17 -O1 -o lz4_host tools/lz4_host.cpp
//   lz4_host corpus.bin
//
// The file holds records: uint64 frame bytes, uint64 out_bytes (little endian), the frame's bytes.  Per record one line:
// status bad_block xxh32-of-the-output blocks_compressed blocks_stored sequences literals matched_bytes content_checksum
// (everything but the first two and the last is 0 for a frame that fails).
#include <cstdio>
#include <cstring>
#include <memory>

#include "../cuttlefish_amd/csrc/lz4.h"

struct Verdict {
	uint32_t status = 0, bad_block = 0, hash = 0, content_checksum = 0;
	uint64_t compressed = 0, stored = 0, sequences = 0, literals = 0, matched = 0;
};

// One compressed block the way the kernel does it: parse a sequence, copy its literals, copy its match byte by byte.
static uint32_t decode_block(const uint8_t* in, uint32_t size, uint8_t* out, uint32_t want, Verdict* v)
{
	uint32_t ip = 0, op = 0;
	uint64_t seqs = 0, lits = 0, matched = 0;
	for (;;) {
		cflz4_seq s;
		const uint32_t e = cflz4_sequence(in, size, want, &ip, op, &s);
		if (e != CFLZ4_OK)
			return e;
		for (uint32_t i = 0; i < s.lit_len; ++i)
			out[op + i] = in[s.lit_at + i];
		op += s.lit_len;
		const uint32_t start = op - s.offset;
		for (uint32_t i = 0; i < s.match_len; ++i)
			out[op + i] = out[start + i % s.offset];
		op += s.match_len;
		++seqs;
		lits += s.lit_len;
		matched += s.match_len;
		if (!s.match_len)
			break;
	}
	if (op != want)
		return CFLZ4_E_SIZE;
	v->sequences += seqs;
	v->literals += lits;
	v->matched += matched;
	return CFLZ4_OK;
}

static Verdict run(const uint8_t* z, uint64_t bytes, uint64_t n)
{
	Verdict v;
	cflz4_header h;
	v.status = cflz4_parse_header(z, bytes, n, &h);
	if (v.status != CFLZ4_OK)
		return v;
	v.content_checksum = h.content_checksum;
	std::unique_ptr<uint8_t[]> out(new uint8_t[n ? n : 1]);
	const uint64_t blocks = (n + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK;
	uint64_t pos = h.length;
	for (uint64_t b = 0; b < blocks; ++b) {
		const uint32_t want = (uint32_t)(n - b*CFLZ4_BLOCK < CFLZ4_BLOCK ? n - b*CFLZ4_BLOCK : CFLZ4_BLOCK);
		uint64_t at = 0;
		uint32_t size = 0, raw = 0;
		v.bad_block = (uint32_t)b;
		v.status = cflz4_next_block(z, bytes, h.block_checksums, &pos, &at, &size, &raw);
		if (v.status != CFLZ4_OK)
			return v;
		if (h.block_checksums && cflz4_le32(z + at + size) != cflz4_xxh32(z + at, size)) {
			v.status = CFLZ4_E_CHECKSUM;
			return v;
		}
		if (raw) {
			if (size != want) {
				v.status = CFLZ4_E_SIZE;
				return v;
			}
			memcpy(out.get() + b*CFLZ4_BLOCK, z + at, size);
			++v.stored;
		} else {
			// the block's bytes in a heap block of their own: a read behind them is a finding
			std::unique_ptr<uint8_t[]> in(new uint8_t[size]);
			memcpy(in.get(), z + at, size);
			v.status = decode_block(in.get(), size, out.get() + b*CFLZ4_BLOCK, want, &v);
			if (v.status != CFLZ4_OK)
				return v;
			++v.compressed;
		}
	}
	v.bad_block = (uint32_t)blocks;
	v.status = cflz4_frame_end(z, bytes, h.content_checksum, pos);
	if (v.status != CFLZ4_OK)
		return v;
	v.bad_block = 0;
	v.hash = cflz4_xxh32(out.get(), (uint32_t)n);
	return v;
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: lz4_host corpus.bin\n");
		return 2;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	uint64_t head[2];
	while (fread(head, 8, 2, f) == 2) {
		if (head[0] > ((uint64_t)1 << 31) || head[1] >= ((uint64_t)1 << 31)) {
			fprintf(stderr, "bad record\n");
			return 2;
		}
		std::unique_ptr<uint8_t[]> z(new uint8_t[head[0] ? head[0] : 1]);
		if (head[0] && fread(z.get(), 1, head[0], f) != head[0]) {
			fprintf(stderr, "truncated record\n");
			return 2;
		}
		const Verdict v = run(z.get(), head[0], head[1]);
		const bool ok = v.status == 0;
		printf("%u %u %u %llu %llu %llu %llu %llu %u\n", v.status, v.bad_block, ok ? v.hash : 0u,
			ok ? (unsigned long long)v.compressed : 0ull, ok ? (unsigned long long)v.stored : 0ull,
			ok ? (unsigned long long)v.sequences : 0ull, ok ? (unsigned long long)v.literals : 0ull,
			ok ? (unsigned long long)v.matched : 0ull, v.content_checksum);
	}
	fclose(f);
	return 0;
}
