// The stage log of the stream codecs' calls (cfhip_api.hip): which event pairs of the context the last call of a family
// took, and which stage each of them times.  No HIP in here: the host compiler builds it alone (tools/stage_log_host.cpp).
//
// A call takes its pairs in one run: `head` pairs once, then `per_slice` pairs for every slice of its input, then `tail`
// pairs once.  Its stages are numbered in that order, a slice's stages once: head + per_slice + tail of them.
#pragma once
#include <stddef.h>

struct StageLog {
	const char* owner;                // the family whose call opened the log (compared by pointer); NULL: closed
	size_t first, pairs;              // the call's event pairs are events[first + 2*i], events[first + 2*i + 1], i < pairs
	size_t head, per_slice, tail;
};

static inline size_t stage_log_stages(const StageLog& g)
{
	return g.head + g.per_slice + g.tail;
}

// A log that a finished call left: head and tail complete, at least one pair, whole slices between them (at least one
// where the family has slices), and every pair still among the context's events in use.
static inline bool stage_log_valid(const StageLog& g, size_t events_used)
{
	if (!g.pairs || g.pairs < g.head + g.tail)
		return false;
	const size_t middle = g.pairs - g.head - g.tail;
	if (g.per_slice ? !middle || middle % g.per_slice : middle != 0)
		return false;
	return g.first + 2*g.pairs <= events_used;
}

// The stage that pair i of a valid log times.
static inline size_t stage_log_stage(const StageLog& g, size_t i)
{
	if (i < g.head)
		return i;
	if (i >= g.pairs - g.tail)
		return stage_log_stages(g) - (g.pairs - i);
	return g.head + (i - g.head) % g.per_slice;
}
