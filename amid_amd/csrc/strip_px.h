// The launches of the backward strips' N-split builds on bf16 pieces (sasrec_strip_px.hip: eight waves per 64-row tile, two per SIMD, each
// owning half the output columns) for the entry points of sasrec_strip.hip, which choose the build by their products-mode argument
// (mma_bf16 = 4).  D = 128; dropout p = 0.5 or none (AMID_ERR_UNSUPPORTED otherwise).  ln_stat / f_ln_stat: the forward's row statistics of
// the q / k / v chain's layer and of the fused feed-forward chain's layer ([2M][4]), or nullptr: the statistics are taken from the rows.
#pragma once
#include "seq_bwd.h"
#include "sort_phases.h"
#include "scorer_sum.h"

namespace amid {

int launch_ffn_bwd_px(const StripFfnBwdArgs& a, const float* ln_stat, const StripGeom& sg, const SortRider& rd, void* stream);
int launch_qkv_bwd_px(const StripQkvBwdArgs& a, const StripFfnBwdArgs& f, bool ffn, const float* ln_stat, const float* f_ln_stat, const ScorerSum& ss,
                      const StripGeom& sg, const SortRider& rd, void* stream);

}  // namespace amid
