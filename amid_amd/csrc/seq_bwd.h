// Arguments of the strip backward chains and of the one-launch backward of a sequence (sasrec_strip.hip: seq_bwd_kernel, a wave per
// 16-row strip; sasrec_seqn_bwd.hip: seqn_bwd_kernel, the N-split build -- two waves share a strip, each owning half the columns).
#pragma once
#include "common.h"
#include "strip_gemm.h"
#include "attention_mfma.h"
#include "host_launch.h"

namespace amid {

struct StripFfnBwdArgs {
    const float* dxo;                   // [2M, D] gradient of the layer output
    const unsigned char* tmq;
    const float* h; const float* r;     // saved relu output, saved LN2 input
    const float* ln_w[2];
    const float* w1T[2]; const float* w2T[2]; const float* woT[2];
    float* dpre2; float* dpre1; float* dr; float* d_o;
    float* ln_part;                     // [2 tpg][2][D]
    float ln_eps;
    const StepState* st; int train; unsigned spec; float scale; int layer;
};

struct StripQkvBwdArgs {
    const float* dq; const float* dk; const float* dv; const float* dr; const float* x;
    const float* ln_w[2];
    const float* wqT[2]; const float* wkT[2]; const float* wvT[2];
    float* dx;
    float* ln_part;                     // [2 tpg][2][D]
    float ln_eps;
    // layer 0's launch of the live-sequence train step (strip_qkv_bwd_kernel without the fused feed-forward): d x is the gradient of the
    // encoder INPUT -- with emb_tmq set the embedding layer's own backward runs on the strip before it is stored (the input dropout's keep
    // bits redrawn, the "== 0" mask, model_seq.py:361-366): what amid_embed_bwd_f32 did in a pass of its own over the stored rows
    const unsigned char* emb_tmq; const StepState* emb_st; int emb_train; unsigned emb_spec; float emb_scale;
};

struct SeqBwdLayer {
    StripFfnBwdArgs f;                  // f.dxo: the top layer's only; f.ln_part / a.ln_part: [2 B][2][D], slot g * B + (index in the domain's live list)
    StripQkvBwdArgs a;                  // a.dx: layer 0's only
    AttnArgs at;
};
struct SeqBwdArgs { SeqBwdLayer L[2]; int n_layers; };

// ---- host side: the feed-forward / out-projection backward of a layer as an entry point states it (the operands of
// amid_sas_strip_ffn_bwd_f32); every field null / zero unless named.  Inside StripQkvBwdCall it is the optional fused block (absent: h == NULL).
struct FfnBwdCall {
    const float* dxo = nullptr; const unsigned char* tmq = nullptr; const float* h = nullptr; const float* r = nullptr;
    FamC ln_w = nullptr, w1T = nullptr, w2T = nullptr, woT = nullptr;
    float ln_eps = 0.f; int layer = 0;
    const void* step_state = nullptr; int train = 0; float p_drop = 0.f;
    float* dpre2 = nullptr; float* dpre1 = nullptr; float* dr = nullptr; float* d_o = nullptr; float* ln_part = nullptr;
    // everything but dxo (a fused block takes its gradient from the chain in front of it)
    bool operands() const { return h && r && ln_w && w1T && w2T && woT && dpre2 && dpre1 && dr && d_o && ln_part && (!train || step_state); }
};
// a record `f` bound to an entry point's parameters of the same names
#define AMID_FFN_BWD_CALL(f)                                                                                                                   \
    FfnBwdCall f;                                                                                                                              \
    f.dxo = dxo; f.tmq = tmq; f.h = h; f.r = r; f.ln_w = ln_w; f.w1T = w1T; f.w2T = w2T; f.woT = woT; f.ln_eps = ln_eps; f.layer = layer;           \
    f.step_state = step_state; f.train = train; f.p_drop = p_drop; f.dpre2 = dpre2; f.dpre1 = dpre1; f.dr = dr; f.d_o = d_o; f.ln_part = ln_part

static inline void fill_ffn_bwd(StripFfnBwdArgs& a, const FfnBwdCall& c) {
    a.dxo = c.dxo; a.tmq = c.tmq; a.h = c.h; a.r = c.r; a.dpre2 = c.dpre2; a.dpre1 = c.dpre1; a.dr = c.dr; a.d_o = c.d_o; a.ln_part = c.ln_part;
    a.ln_eps = c.ln_eps; a.st = (const StepState*)c.step_state; a.layer = c.layer;
    const DropoutArgs d = dropout_args(c.train, c.p_drop);
    a.train = d.train; a.spec = d.spec; a.scale = d.scale;
    for (int g = 0; g < 2; ++g) { a.ln_w[g] = c.ln_w[g]; a.w1T[g] = c.w1T[g]; a.w2T[g] = c.w2T[g]; a.woT[g] = c.woT[g]; }
}

// the N-split build of the one-launch backward (sasrec_seqn_bwd.hip); AMID_ERR_UNSUPPORTED when it does not cover the arguments
int launch_seqn_bwd(const SeqBwdArgs& a, const StripGeom& sg, int D, int mma_bf16, void* stream);

}  // namespace amid
