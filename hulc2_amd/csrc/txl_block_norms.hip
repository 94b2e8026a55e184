// txl_block_norms.hip — the whole-trunk launches (txl_block.hip) with the two optional LayerNorms of the plan-recognition transformer:
//     positional_normalize: x0 = dropout(LN_pos(emb + pos[arange(S)]))        (plan_recognition_net.py:140-142)
//     encoder_normalize:    nn.TransformerEncoder(norm = LN_enc) ahead of the mean over S   (plan_recognition_net.py:118-121)
// Both sit at the ends of the trunk, where the launches have a per-sequence stage anyway: LN_pos replaces the position add of the forward
// (wave w normalises rows w, w + 4, ..) and follows the dropout backward in front of demb; LN_enc normalises the last layer's rows where
// they lie in LDS for the pool, and backward sends dpooled / S through it ahead of the last layer.  Both backward stages are ln_bwd_regs in
// the register layout of the stages next to them.  Shared sequences: every member computes both stages (identical values), no exchange is
// added or moved.  Kernels of their own (and a translation unit of their own, see txl_block.h): the plain launches keep their code.
#include "txl_block.h"

namespace {

// operands of the two optional LayerNorm stages (txl_block_norms.hip; they cross the C ABI by value)
struct NormP {
    const float *pos_g, *pos_b;                      // (E,) LN_pos weight / bias; null = stage off
    float *pre0, *mean0, *rstd0;                     // kept: (T, E), (T,), (T,)
    float* lnp0;                                     // backward out: (B, 2, E)
    const float *enc_g, *enc_b;                      // (E,) LN_enc weight / bias; null = stage off
    float *meanF, *rstdF;                            // kept: (T,), (T,)
    float* lnpF;                                     // backward out: (B, 2, E)
};

// statistics of one 128-wide row held two features per lane by one wave: the two-pass form of the layers' LayerNorms
HULC_DEVICE void row_stats(float a, float c, float eps, float& mean, float& rstd) {
    mean = wave_sum(a + c) * (1.0f / E);
    const float da = a - mean, dc = c - mean;
    rstd = rsqrtf(wave_sum(da * da + dc * dc) * (1.0f / E) + eps);
}

// positional_normalize: x0 = dropout(LN_pos(emb + pos[pos_ids[s]])), pos_add_seq's dropout stream and element index.  Wave w takes rows
// w, w + 4, .. < S; pre0 = emb + pos and the statistics are kept for backward (all three or none)
HULC_DEVICE void pos_norm_seq(const BlockP& d, const NormP& n, int b) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = d.S, c = 2 * lane;
    const unsigned long long seed = d.seed_pos ^ (d.seed_dev ? d.seed_dev[0] : 0ull);
    float* x0 = d.layers[0].x;
    const float2 gm = *(const float2*)(n.pos_g + c), bt = *(const float2*)(n.pos_b + c);
    for (int s = w; s < S; s += 4) {
        const long tok = (long)b * S + s, i = tok * E + c;
        const float2 a = *(const float2*)(d.emb + i), q = *(const float2*)(d.pos + d.pos_ids[s] * E + c);
        const float v0 = a.x + q.x, v1 = a.y + q.y;
        float mean, rstd;
        row_stats(v0, v1, d.eps, mean, rstd);
        float y0 = (v0 - mean) * rstd * gm.x + bt.x, y1 = (v1 - mean) * rstd * gm.y + bt.y;
        if (d.drop_p > 0.f) { y0 *= dropout_scale(seed, (uint64_t)i, d.drop_p); y1 *= dropout_scale(seed, (uint64_t)(i + 1), d.drop_p); }
        *(float2*)(x0 + i) = make_float2(y0, y1);
        if (n.pre0) {
            *(float2*)(n.pre0 + i) = make_float2(v0, v1);
            if (lane == 0) { n.mean0[tok] = mean; n.rstd0[tok] = rstd; }
        }
    }
}

// encoder_normalize: the last layer's rows, left in LDS for the sequence mean (rows[s][E], s < S), are normalised in place
HULC_DEVICE void enc_norm_rows(const BlockP& d, const NormP& n, int b, float* rows) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = d.S, c = 2 * lane;
    const float2 gm = *(const float2*)(n.enc_g + c), bt = *(const float2*)(n.enc_b + c);
    for (int s = w; s < S; s += 4) {
        const float2 v = *(const float2*)(rows + s * E + c);
        float mean, rstd;
        row_stats(v.x, v.y, d.eps, mean, rstd);
        *(float2*)(rows + s * E + c) = make_float2((v.x - mean) * rstd * gm.x + bt.x, (v.y - mean) * rstd * gm.y + bt.y);
        if (n.meanF && lane == 0) { n.meanF[(long)b * S + s] = mean; n.rstdF[(long)b * S + s] = rstd; }
    }
}

// the forward launch with the optional LayerNorm stages (n.pos_g / n.enc_g non-null = that stage is on).  
template <bool X3>
__global__ __launch_bounds__(256) void txl_block_norms_fwd_kernel(BlockK k, NormP n) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const BlockP& d = k.d;
    const int tid = threadIdx.x;
    int b, q;
    if (!quad_ids(k, b, q)) return;
    if (n.pos_g) pos_norm_seq(d, n, b);
    else pos_add_seq(d, b);
    __syncthreads();
    for (int li = 0; li < d.L; ++li) {
        const LayerP& l = d.layers[li];
        const TxlP p = attn_params(d, l);
        // (the sequence index is made opaque per layer: otherwise the compiler hoists every layer-invariant piece of the dropout hashes and
        // address products out of this loop — 60+ registers live across both stages, spilled)
        int bb = b;
        asm volatile("" : "+s"(bb));
        txl_attn_fwd_body<X3>(p, bb, lds);
        __syncthreads();
        ffn_fwd_seq<X3>(k, l, bb, q, li, lds, li + 1 == d.L);
        __syncthreads();
    }
    quad_finish(k, b);
    if (n.enc_g) {                                                  // every member normalises its own copy of the rows (identical values)
        enc_norm_rows(d, n, b, (float*)lds);
        __syncthreads();
    }
    if (d.pooled && tid < E) {                                      // seq_mean_fwd_kernel's summation order, rows from LDS
        const float* xb = (const float*)lds + tid;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int t = 0;
        for (; t + 3 < d.S; t += 4) {
            const float a = xb[(long)t * E], c = xb[(long)(t + 1) * E], e = xb[(long)(t + 2) * E], f = xb[(long)(t + 3) * E];
            s0 += a; s1 += c; s2 += e; s3 += f;
        }
        for (; t < d.S; ++t) s0 += xb[(long)t * E];
        d.pooled[(long)b * E + tid] = ((s0 + s1) + (s2 + s3)) / d.S;
    }
}

// the backward launch with the optional LayerNorm stages
__global__ __launch_bounds__(256) void txl_block_norms_bwd_kernel(BlockK k, NormP n) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const BlockP& d = k.d;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hf = lane >> 5;
    int b, q;
    if (!quad_ids(k, b, q)) return;
    const int S = d.S;
    const long tok0 = (long)b * S;
    const bool live = r < S;
    const long off = (tok0 + (live ? r : 0)) * E + 32 * w + 4 * hf;
    // (the LayerNorm stages of the launch with norms: ffn_bwd_seq's places for the transposes and the row sums)
    float (*lt)[2][32][33] = (float (*)[2][32][33])(lds + 8 * 2 * 32 * 16);
    float (*red)[4][32] = (float (*)[4][32])(lds + PART_BYTES);
    float dyv[16];                                                  // gradient of the current layer's output: registers from stage to stage
    {                                                               // mean over the sequence: every token receives dpooled / S
        const float* src = d.dpooled + (long)b * E + 32 * w + 4 * hf;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 a = *(const float4*)(src + 8 * q4);
            dyv[4 * q4] = a.x / S; dyv[4 * q4 + 1] = a.y / S; dyv[4 * q4 + 2] = a.z / S; dyv[4 * q4 + 3] = a.w / S;
        }
        if (!live) {
#pragma unroll
            for (int e = 0; e < 16; ++e) dyv[e] = 0.f;
        }
    }
    if (n.enc_g) {                                         // encoder_normalize: through LN_enc of the last layer's y2 (dead lanes carry zeros)
        float dpre[16];
        ln_bwd_regs(dyv, d.layers[d.L - 1].y2, n.meanF, n.rstdF, n.enc_g, tok0 + (live ? r : 0), b, lt, red, n.lnpF, dpre);
#pragma unroll
        for (int e = 0; e < 16; ++e) dyv[e] = live ? dpre[e] : 0.f;
        __syncthreads();
    }
    for (int li = d.L - 1; li >= 0; --li) {
        const LayerP& l = d.layers[li];
        int bb = b;                                                 // (opaque per layer, see the forward kernel)
        asm volatile("" : "+s"(bb));
        float dy1[16];
        ffn_bwd_seq(k, l, bb, q, li, dyv, dy1, lds);
        __syncthreads();
        const TxlP p = attn_params(d, l);
        asm volatile("" : "+s"(bb));
        txl_attn_bwd_body<true>(p, bb, lds, dy1, dyv);
        __syncthreads();
    }
    quad_finish(k, b);
    if (n.pos_g) {                                         // positional_normalize: dropout backward, then through LN_pos of pre0
        const unsigned long long seed = d.seed_pos ^ (d.seed_dev ? d.seed_dev[0] : 0ull);
        float keep[16], dpre[16];
        if (d.drop_p > 0.f) dropout_scale_acc16(seed, (uint64_t)((tok0 + r) * E + 32 * w), hf, d.drop_p, keep);
#pragma unroll
        for (int e = 0; e < 16; ++e) dyv[e] = !live ? 0.f : d.drop_p > 0.f ? dyv[e] * keep[e] : dyv[e];
        ln_bwd_regs(dyv, n.pre0, n.mean0, n.rstd0, n.pos_g, tok0 + (live ? r : 0), b, lt, red, n.lnp0, dpre);
        if (live) {
            float* dst = d.demb + off;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) *(float4*)(dst + 8 * q4) = make_float4(dpre[4 * q4], dpre[4 * q4 + 1], dpre[4 * q4 + 2], dpre[4 * q4 + 3]);
        }
        return;
    }
    if (live) {                                                     // dropout of the position-embedded input (dropout_bwd_kernel's stream)
        const unsigned long long seed = d.seed_pos ^ (d.seed_dev ? d.seed_dev[0] : 0ull);
        float* dst = d.demb + off;
        float keep[16];
        if (d.drop_p > 0.f) dropout_scale_acc16(seed, (uint64_t)((tok0 + r) * E + 32 * w), hf, d.drop_p, keep);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            float4 a = make_float4(dyv[4 * q4], dyv[4 * q4 + 1], dyv[4 * q4 + 2], dyv[4 * q4 + 3]);
            if (d.drop_p > 0.f) { a.x *= keep[4 * q4]; a.y *= keep[4 * q4 + 1]; a.z *= keep[4 * q4 + 2]; a.w *= keep[4 * q4 + 3]; }
            *(float4*)(dst + 8 * q4) = a;
        }
    }
}

// the optional LayerNorm stages: what the launch with norms adds to block_check
int norms_check(const NormP* n, bool bwd) {
    if ((n->pos_g != nullptr) != (n->pos_b != nullptr) || (n->enc_g != nullptr) != (n->enc_b != nullptr))
        return hulc_fail(-3, "hulc_txl_block_norms: gamma and beta of a stage come together");
    if (n->pos_g && ((n->pre0 != nullptr) != (n->mean0 != nullptr) || (n->mean0 != nullptr) != (n->rstd0 != nullptr)))
        return hulc_fail(-3, "hulc_txl_block_norms: pre0 / mean0 / rstd0 are kept together or not at all");
    if (n->enc_g && (n->meanF != nullptr) != (n->rstdF != nullptr))
        return hulc_fail(-3, "hulc_txl_block_norms: meanF / rstdF are kept together or not at all");
    if (bwd && ((n->pos_g && (!n->pre0 || !n->mean0 || !n->rstd0 || !n->lnp0)) || (n->enc_g && (!n->meanF || !n->rstdF || !n->lnpF))))
        return hulc_fail(-1, "hulc_txl_block_norms_bwd: an enabled stage needs its kept statistics and its partial buffer");
    return 0;
}

}  // namespace

// see include/hulc2_amd.h
extern "C" int hulc_txl_block_norms_fwd(const hulc_txl_block_desc* d, const float* pos_g, const float* pos_b, float* pre0, float* mean0, float* rstd0,
                                        const float* enc_g, const float* enc_b, float* meanF, float* rstdF, void* stream) {
    const NormP nv = {pos_g, pos_b, pre0, mean0, rstd0, nullptr, enc_g, enc_b, meanF, rstdF, nullptr};
    const NormP* n = &nv;
    if (int rc = block_check(d, false, "hulc_txl_block_norms_fwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands")) return rc;
    if (int rc = norms_check(n, false)) return rc;
    if (!n->pos_g && !n->enc_g) return hulc_txl_block_fwd(d, stream);
    static bool attr = false;
    if (!attr) {
        if (int rc = block_lds((const void*)txl_block_norms_fwd_kernel<false>)) return rc;
        if (int rc = block_lds((const void*)txl_block_norms_fwd_kernel<true>)) return rc;
        attr = true;
    }
    int nlo = 0;
    if (int rc = block_split_layers(d, nlo)) return rc;
    const int Q = block_share(d);
    const unsigned grid = Q == 1 ? (unsigned)d->B : (unsigned)((d->B + 7) / 8 * 8 * Q);
    if (nlo) txl_block_norms_fwd_kernel<true><<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q), *n);
    else txl_block_norms_fwd_kernel<false><<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q), *n);
    return hulc_check_launch("hulc_txl_block_norms_fwd");
}

extern "C" int hulc_txl_block_norms_bwd(const hulc_txl_block_desc* d, const float* pos_g, const float* pos_b, const float* pre0, const float* mean0,
                                        const float* rstd0, float* lnp0, const float* enc_g, const float* enc_b, const float* meanF,
                                        const float* rstdF, float* lnpF, void* stream) {
    const NormP nv = {pos_g, pos_b, (float*)pre0, (float*)mean0, (float*)rstd0, lnp0, enc_g, enc_b, (float*)meanF, (float*)rstdF, lnpF};
    const NormP* n = &nv;
    if (int rc = block_check(d, true, "hulc_txl_block_norms_bwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands")) return rc;
    if (!d->dpooled || !d->demb) return hulc_fail(-1, "hulc_txl_block_norms_bwd: null pointer");
    if (int rc = norms_check(n, true)) return rc;
    if (!n->pos_g && !n->enc_g) return hulc_txl_block_bwd(d, stream);
    static bool attr = false;
    if (!attr) { if (int rc = block_lds((const void*)txl_block_norms_bwd_kernel)) return rc; attr = true; }
    const int Q = block_share(d);
    const unsigned grid = Q == 1 ? (unsigned)d->B : (unsigned)((d->B + 7) / 8 * 8 * Q);
    txl_block_norms_bwd_kernel<<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q), *n);
    return hulc_check_launch("hulc_txl_block_norms_bwd");
}
