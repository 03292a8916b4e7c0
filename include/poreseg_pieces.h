/*
 * poreseg_pieces.h -- the general form of libporeseg.so's event detector: every piece a threshold cuts a trace into, with its
 * statistics (ps_detect_pieces).  An extension beside poreseg.h, as poreseg_comm.h is: poreseg.h holds the entry points
 * that replace the reference's interface one for one; this call serves rules of the caller's own
 * (lambda_event_parser(threshold, rules=[...], on_device=True)).  Same library, same context, same status codes.
 */
#ifndef PORESEG_PIECES_H
#define PORESEG_PIECES_H

#include "poreseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The general form of the detector, for rules of the caller's own (lambda_event_parser(threshold, rules=[...])): EVERY piece
 * the threshold cuts the trace into, with its statistics, on the device.  Sample i is below when double(k_i) * quantum <
 * threshold (k_i: the count, offset_counts included; the predicate of ps_detect_events); an edge sits at i >= 1 when below(i) !=
 * below(i - 1); with the edges e_1 < ... < e_{P-1}, e_0 = 0 and e_P = n, piece p is [e_p, e_{p+1}).  P = 1 + the number of edges;
 * n == 0 gives P = 0.  Device outputs, ascending: d_edges[0 .. P] (cap + 1 entries; d_edges[P] = n) and one ps_segstat per piece
 * in d_stats (cap entries), by the definition of ps_range_stats in poreseg.h -- k0 the count of the piece's first sample, exact integer
 * sums of k - k0 and (k - k0)^2, the same final expressions, so ps_range_stats on [e_p, e_{p+1}) gives the same bits.
 * *n_pieces_out is always P; P > cap: PS_ERR_CAPACITY, the tables undefined (call again with room for P).  int16 counts or
 * float32 on the grid; n <= 2^31 - 1.  Refused: any other dtype, a float32 sample off the grid or with |count| >= 2^23
 * (PS_ERR_OFF_GRID), and a float32 sample so far from its piece's first that n (k - k0)^2 could leave int64 (PS_ERR_ARG, "counts
 * too wide"; int16 counts cannot).  That bound is set by the length of the whole TRACE, floor(sqrt((2^63 - 1) / n)) counts -- 2^24
 * up to 2^15 samples, about 3e5 at 1e8 --, whatever the pieces' own lengths: a float32 trace of short pieces whose levels lie
 * further apart is refused here and can be served by ps_range_stats on edges found otherwise.  Two passes over the samples and a scan over their 4096-sample chunks: four launches and ONE
 * host synchronisation whatever P is, one status word.  Nothing depends on launch shape or arrival order: no float
 * accumulation, no atomics on results.  The scratch belongs to the context and is freed with it. */
int ps_detect_pieces(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, double threshold,
                     int64_t *d_edges /* cap + 1 */, ps_segstat *d_stats /* cap */, int64_t cap, int64_t *n_pieces_out);

#ifdef __cplusplus
}
#endif
#endif /* PORESEG_PIECES_H */
