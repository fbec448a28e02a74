// The stage log's two pure functions (csrc/stage_log.h) on the CPU, for tests/test_stage_log_host.py.
// usage: stage_log_host <head> <per_slice> <tail> <first> <pairs> <events_used> ...   (any number of such groups)
// One line per group: "0" for a log that is not valid, else "1" and the stage of every pair.
#include <cstdio>
#include <cstdlib>

#include "../cuttlefish_amd/csrc/stage_log.h"

int main(int argc, char** argv)
{
	if (argc < 7 || (argc - 1) % 6) {
		fprintf(stderr, "usage: %s <head> <per_slice> <tail> <first> <pairs> <events_used> ...\n", argv[0]);
		return 2;
	}
	for (int a = 1; a < argc; a += 6) {
		size_t v[6];
		for (int k = 0; k < 6; ++k)
			v[k] = (size_t)strtoull(argv[a + k], nullptr, 10);
		const StageLog g = {"family", v[3], v[4], v[0], v[1], v[2]};
		if (!stage_log_valid(g, v[5])) {
			puts("0");
			continue;
		}
		printf("1");
		for (size_t i = 0; i < g.pairs; ++i) {
			const size_t s = stage_log_stage(g, i);
			if (s >= stage_log_stages(g)) {
				fprintf(stderr, "pair %zu maps to stage %zu of %zu\n", i, s, stage_log_stages(g));
				return 1;
			}
			printf(" %zu", s);
		}
		printf("\n");
	}
	return 0;
}
