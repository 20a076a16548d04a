// Call scatter (scatter.hip, ops/scatter.py): Q questions expanded into T calls on the
// device -- the scatter half of a scatter-gather (the reference's splitWork,
// example/optimus/coordinator.go:67-73, for any step, and a broadcast to a group).
//
// Question q becomes n[q] >= 0 rows; first[q] is the exclusive prefix of n, so q owns
// the rows first[q] .. first[q] + n[q] - 1, in question order.  With k = row - first[q]:
//   ranges   t = a0[q]; n = t <= 0 ? 0 : (t - 1) / step + 1 (unsigned);
//            actor = (actor_base + row) % n_actors, a0 = k * step (first_lo at k == 0
//            when one is given), a1 = (k + 1) * step, a2 = t
//   members  g = actor[q] names a group of the CSR (offsets int64[G + 1], members
//            int32[offsets[G]]); n = offsets[g + 1] - offsets[g], 0 for g outside [0, G)
//            (counted in `oob`); actor = members[offsets[g] + k], a0 / a1 / a2 the question's
//   topics   g = actor[q] names a topic of a segment table (ops/topics.py): topic g owns the
//            segments seg_off[g] .. seg_off[g + 1] - 1 (seg_off int64[G + 1]); segment s is the
//            actors seg_start[s] + seg_stride[s] * j, 0 <= j < row_off[s + 1] - row_off[s]
//            (row_off int64[S + 1], the exclusive prefix of the segment counts, every count
//            >= 1; seg_start / seg_stride int32[S]).  n = row_off[seg_off[g + 1]] -
//            row_off[seg_off[g]], 0 for g outside [0, G) (counted in `oob`); row k belongs to
//            the segment s of g with row_off[s] <= row_off[seg_off[g]] + k < row_off[s + 1];
//            a0 / a1 / a2 the question's.  No per-subscriber table exists.
//            Queue subscriptions (competing consumers): the table may also hold NQ of them, their
//            segments after the S ordinary ones in row_off / seg_start / seg_stride (seg_off[G]
//            = S keeps bounding the ordinary ones).  Topic g owns the queue subscriptions
//            q_off[g] .. q_off[g + 1] - 1 (q_off int64[G + 1]), queue subscription j the segments
//            q_seg[j] .. q_seg[j + 1] - 1 (q_seg int64[NQ + 1], 1 to 1024 each) and their
//            c = row_off[q_seg[j + 1]] - row_off[q_seg[j]] members, 1 <= c <= 2^31 - 1.  After
//            its ordinary rows a question has ONE row per queue subscription of its topic, in
//            q_off's order: n grows by q_off[g + 1] - q_off[g].  That row goes to member
//              by key    m = ((mix64(key[q]) >> 32) * c) >> 32   (u64; key int64[Q]; mix64 of common.hpp)
//              by index  m = ((seq + q) mod 2^64) mod c           (seq: a u64 of the caller's)
//            of the subscription: the segment s with row_off[s] <= row_off[q_seg[j]] + m <
//            row_off[s + 1].  A compile-time variant of this rule, launched only for a table
//            with NQ >= 1; a table without one runs the kernels it always ran.
// The method is the question's (one id, or an int16 column copied per row); `group`
// holds the question index of every row.
//
// Counters (u64): [0] the total, saturating at 2^64 - 1; [1] oob.  The host reads
// both before the expand pass is launched, so no row is written past the capacity.
#pragma once
#include <stdint.h>

namespace ptype {

constexpr int kScatterRanges = 0;
constexpr int kScatterMembers = 1;
constexpr int kScatterTopics = 2;
constexpr int kScatterRules = 3;

constexpr int kScatterCtrWords = 2;
// rows of one expansion: a Gather takes M < 2^31 - 1 replies
constexpr int64_t kScatterMaxRows = 0x7ffffffell;
constexpr int64_t kScatterMaxQuestions = 1ll << 26;
constexpr int64_t kScatterMaxStep = 0x7fffffffll;
// segments of one topic table: a segment index fits the int of the owner search
constexpr int64_t kScatterMaxSegments = 1ll << 24;
// queue subscriptions of one topic table
constexpr int64_t kScatterMaxQueues = 1ll << 24;

}  // namespace ptype
