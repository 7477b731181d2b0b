// What dmff_fused.hip (two-launch form) and dmff_wide.hip (three-launch form) share on the host: both read one icaf_dmff_args.
#pragma once
#include "icaf_common.h"

namespace icaf {

// The fields DmffP and WideP have in common, under the same member names; each file's fill adds what is its own.
template <class P>
static inline void dmff_fill_common(const icaf_dmff_args* a, P& p) {
    p.x = a->x; p.qkv = a->qkv; p.y = a->y;
    p.wqkv = a->wqkv; p.bqkv = a->bqkv; p.wo = a->wo; p.bo = a->bo; p.w1 = a->w1; p.b1 = a->b1; p.w2 = a->w2; p.b2 = a->b2;
    p.ln_a_g[0] = a->ln_attn_gamma[0]; p.ln_a_g[1] = a->ln_attn_gamma[1]; p.ln_a_b[0] = a->ln_attn_beta[0]; p.ln_a_b[1] = a->ln_attn_beta[1];
    p.ln_m_g = a->ln_mlp_gamma; p.ln_m_b = a->ln_mlp_beta;
    p.wqkv_gs = a->wqkv_gs; p.bqkv_gs = a->bqkv_gs; p.wo_gs = a->wo_gs; p.bo_gs = a->bo_gs; p.w1_gs = a->w1_gs; p.b1_gs = a->b1_gs;
    p.w2_gs = a->w2_gs; p.b2_gs = a->b2_gs; p.x_gs = a->x_gs; p.y_gs = a->y_gs;
    p.C = a->C; p.Kp = a->Kp; p.Kp4 = a->Kp4; p.hid = a->hidden; p.ldy = a->ldy;
    p.eps_a = a->eps_attn; p.eps_m = a->eps_mlp;
    for (int g = 0; g < 2; ++g) {
        p.c_res_a[g] = a->coef_res_attn[g]; p.c_acc_a[g] = a->coef_acc_attn[g];
        p.c_res_m[g] = a->coef_res_mlp[g]; p.c_acc_m[g] = a->coef_acc_mlp[g];
    }
}

// dmff_fused.hip: the two-launch form (icaf_dmff_ln_qkv + icaf_dmff_attn_mlp) covers this shape — the verdict of the resolve its launches run
bool dmff_fused_covered(int dtype, int C, int N, int heads, int hidden);

}  // namespace icaf
