/* The layout of the nine public structs of include/poreseg.h as the C compiler sees it: one line "struct sizeof N" per struct
   and one line "struct.field N" per field, in declaration order.  tests/test_binding_host.py compares the lines with the
   ctypes structures of pypore_amd/_lib.py.  Behind them the indices of what ps_get_timings returns, one line "NAME enum N" each,
   in the header's order, which the test compares with the two tuples of names of _lib.py.  Plain C, needs only -Iinclude. */
#include <stddef.h>
#include <stdio.h>

#include "poreseg.h"

#define SIZE(T) printf(#T " sizeof %zu\n", sizeof(T))
#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define ENUM(e) printf(#e " enum %d\n", (int)(e))

int main(void) {
    SIZE(ps_split_params);
    FIELD(ps_split_params, min_width); FIELD(ps_split_params, max_width); FIELD(ps_split_params, window_width);
    FIELD(ps_split_params, min_gain_per_sample); FIELD(ps_split_params, false_positive_rate);
    FIELD(ps_split_params, prior_segments_per_second); FIELD(ps_split_params, sampling_freq); FIELD(ps_split_params, cutoff_freq);

    SIZE(ps_sample_format);
    FIELD(ps_sample_format, dtype); FIELD(ps_sample_format, offset_counts); FIELD(ps_sample_format, quantum);

    SIZE(ps_pool_plan_t);
    FIELD(ps_pool_plan_t, n_eff); FIELD(ps_pool_plan_t, k0_waves); FIELD(ps_pool_plan_t, k0_admit); FIELD(ps_pool_plan_t, lat_help);

    SIZE(ps_statsplit_params);
    FIELD(ps_statsplit_params, min_width); FIELD(ps_statsplit_params, max_width); FIELD(ps_statsplit_params, window_width);
    FIELD(ps_statsplit_params, threshold); FIELD(ps_statsplit_params, use_log); FIELD(ps_statsplit_params, splitter);

    SIZE(ps_grid_report);
    FIELD(ps_grid_report, max_frac); FIELD(ps_grid_report, min_frac_above); FIELD(ps_grid_report, min_count);
    FIELD(ps_grid_report, max_count); FIELD(ps_grid_report, n_nonfinite); FIELD(ps_grid_report, n_undefined);

    SIZE(ps_hmm_model);
    FIELD(ps_hmm_model, n_states); FIELD(ps_hmm_model, n_emit); FIELD(ps_hmm_model, n_levels); FIELD(ps_hmm_model, start);
    FIELD(ps_hmm_model, end); FIELD(ps_hmm_model, finite); FIELD(ps_hmm_model, kind); FIELD(ps_hmm_model, level_ptr);
    FIELD(ps_hmm_model, in_ptr); FIELD(ps_hmm_model, in_src); FIELD(ps_hmm_model, out_ptr); FIELD(ps_hmm_model, out_dst);
    FIELD(ps_hmm_model, param); FIELD(ps_hmm_model, in_lp); FIELD(ps_hmm_model, out_lp); FIELD(ps_hmm_model, kde_ptr);
    FIELD(ps_hmm_model, kde_pt); FIELD(ps_hmm_model, kde_lw); FIELD(ps_hmm_model, n_dim); FIELD(ps_hmm_model, comp_kind);
    FIELD(ps_hmm_model, comp_param); FIELD(ps_hmm_model, comp_w); FIELD(ps_hmm_model, mix_ptr); FIELD(ps_hmm_model, mix_kind);
    FIELD(ps_hmm_model, mix_param); FIELD(ps_hmm_model, mix_lw); FIELD(ps_hmm_model, mix_cdf); FIELD(ps_hmm_model, mix_draw);

    SIZE(ps_hmm_sample_tables);
    FIELD(ps_hmm_sample_tables, out_cdf); FIELD(ps_hmm_sample_tables, emit_param); FIELD(ps_hmm_sample_tables, kde_cdf);
    FIELD(ps_hmm_sample_tables, n_cdf); FIELD(ps_hmm_sample_tables, n_param); FIELD(ps_hmm_sample_tables, n_kde);

    SIZE(ps_near_tie);
    FIELD(ps_near_tie, event); FIELD(ps_near_tie, window_start); FIELD(ps_near_tie, window_end); FIELD(ps_near_tie, split);

    SIZE(ps_filter_derivative_params);
    FIELD(ps_filter_derivative_params, low_threshold); FIELD(ps_filter_derivative_params, high_threshold);
    FIELD(ps_filter_derivative_params, cutoff_freq); FIELD(ps_filter_derivative_params, sampling_freq);
    FIELD(ps_filter_derivative_params, prefiltered);

    ENUM(PS_MS_SPINE); ENUM(PS_MS_TREE); ENUM(PS_MS_GATHER); ENUM(PS_MS_TOTAL); ENUM(PS_MS_STITCH); ENUM(PS_MS_BRIDGE); ENUM(PS_MS_BLOCKSUM);
    ENUM(PS_MS_SEQ); ENUM(PS_MS_COUNT);
    ENUM(PS_CNT_WINDOWS); ENUM(PS_CNT_CANDIDATES); ENUM(PS_CNT_TILES); ENUM(PS_CNT_TREE_JOBS); ENUM(PS_CNT_REPAIRS); ENUM(PS_CNT_EXACT_RESCANS);
    ENUM(PS_CNT_FULL_EXACT_SCANS); ENUM(PS_CNT_WIDE_REDO); ENUM(PS_CNT_WINDOWS_SPINE); ENUM(PS_CNT_WINDOWS_BRIDGE); ENUM(PS_CNT_WINDOWS_TREE);
    ENUM(PS_CNT_NEAR_TIES); ENUM(PS_CNT_HELPER_CHUNKS_PUBLISHED); ENUM(PS_CNT_HELPER_CHUNKS_TAKEN); ENUM(PS_CNT_TREE_DEFERRED);
    ENUM(PS_CNT_WINDOWS_SCREEN); ENUM(PS_CNT_LOOKAHEAD_SKIPPED); ENUM(PS_CNT_UPLOAD_SKIPPED); ENUM(PS_CNT_SEAMS_RESUMED); ENUM(PS_CNT_COUNT);
    return 0;
}
