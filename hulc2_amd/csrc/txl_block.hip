// txl_block.hip — the plan-recognition transformer trunk as ONE launch per direction (bf16 MFMA).
//
// reference arithmetic: PlanRecognitionTransformersNetwork.forward up to the sequence mean, hulc2/models/plan_encoders/plan_recognition_net.py:125-146 —
//     x0 = dropout(emb + pos[arange(S)]);  L x nn.TransformerEncoderLayer (post-norm, d_model 128, 8 heads, ReLU feed-forward, dropout p);  mean over S
// and its autograd backward.  Everything up to the mean is independent per sequence, so one workgroup (4 waves) owns one sequence for the
// whole trunk: the attention halves are the bodies of hulc_txl_attn_fwd / _bwd (txl_attn.h), the feed-forward halves are new here.
//
// Feed-forward half on 32 tokens without LDS traffic in its loop: wave w owns 32 of every 128 hidden units.  It computes the TRANSPOSED
// hidden tile z^T[hidden][token] = W1s y1^T (accumulator: lane <-> token, registers <-> hidden units), applies bias / ReLU / dropout in
// registers, and — the accumulator-as-operand trick of txl_fused.hip — feeds the packed tile straight back as the B operand of
// f^T[out][token] += W2[out][hidden] h^T[hidden][token] with W2's columns read in the register order.  Four 32-row output tiles accumulate
// over all hidden units of the wave; the four waves' partial tiles meet once per layer in LDS (fixed order), after which wave w holds
// output features 32w.. in exactly the (lane <-> token, registers <-> features) layout the residual + dropout + LayerNorm epilogue of the
// attention half uses.  Backward is the mirror image: z^T recomputed, dh^T = (W2^T df^T) * gate, dy1^T += W1^T dh^T accumulated in registers,
// h and dh stored once (bf16, token-major) as the operands of the weight-gradient products, which join the pass's grouped launch
// (wgrad_group.hip) together with the attention half's.
//
// Stages hand tensors to each other through memory that backward keeps anyway (y1, y2, ...): written and re-read by the same workgroup
// (same CU, L1 / L2 resident) with a workgroup barrier in between.
//
// One workgroup per sequence uses B of the 256 CUs, and the feed-forward half is most of the work (2 x 2048 x 128 MACs and 2048 dropout
// draws per token).  While B Q <= 256, Q = 2 or 4 workgroups SHARE a sequence: each runs the (cheap) attention half redundantly — same
// inputs, same instructions, the same bits — and takes 1 / Q of the hidden units in the feed-forward half; the Q partial output tiles
// (32 x 128 fp32) are exchanged through memory (write-through stores, one arrival counter per sequence, plain loads from a region used
// once per launch: the protocol of mlp_chain.hip) and summed in workgroup order by all Q, which then continue in lock step.  Tensors every
// member computes are stored by every member (identical values).  Like mlp_chain this needs its workgroups co-resident: the launcher picks
// Q > 1 only when the whole grid fits the device, and a member that waits too long sets bit 2 of the sticky fault word.
//
// The stages and the launchers' helpers are in txl_block.h; txl_block_norms.hip adds the launches with the two optional LayerNorms.
#include "txl_block.h"

namespace {

template <bool X3>
__global__ __launch_bounds__(256) void txl_block_fwd_kernel(BlockK k) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const BlockP& d = k.d;
    const int tid = threadIdx.x;
    int b, q;
    if (!quad_ids(k, b, q)) return;
    pos_add_seq(d, b);
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

__global__ __launch_bounds__(256) void txl_block_bwd_kernel(BlockK k) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const BlockP& d = k.d;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hf = lane >> 5;
    int b, q;
    if (!quad_ids(k, b, q)) return;
    const int S = d.S;
    const long tok0 = (long)b * S;
    const bool live = r < S;
    const long off = (tok0 + (live ? r : 0)) * E + 32 * w + 4 * hf;
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

}  // namespace

// see include/hulc2_amd.h
extern "C" long hulc_txl_block_workspace(int B, int L) {
    return SYNC_BYTES + (long)L * B * 4 * (4 * 16 * 64) * 4;
}

extern "C" int hulc_txl_block_fwd(const hulc_txl_block_desc* d, void* stream) {
    if (int rc = block_check(d, false, "hulc_txl_block_fwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands")) return rc;
    static bool attr = false;
    if (!attr) {
        if (int rc = block_lds((const void*)txl_block_fwd_kernel<false>)) return rc;
        if (int rc = block_lds((const void*)txl_block_fwd_kernel<true>)) return rc;
        attr = true;
    }
    int nlo = 0;
    if (int rc = block_split_layers(d, nlo)) return rc;
    const int Q = block_share(d);
    const unsigned grid = Q == 1 ? (unsigned)d->B : (unsigned)((d->B + 7) / 8 * 8 * Q);
    if (nlo) txl_block_fwd_kernel<true><<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q));
    else txl_block_fwd_kernel<false><<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q));
    return hulc_check_launch("hulc_txl_block_fwd");
}

extern "C" int hulc_txl_block_bwd(const hulc_txl_block_desc* d, void* stream) {
    if (int rc = block_check(d, true, "hulc_txl_block_bwd: needs d_model 128, 8 heads, 1 <= S <= 32, 1 <= L <= 4, FF a multiple of 128 and non-null operands")) return rc;
    if (!d->dpooled || !d->demb) return hulc_fail(-1, "hulc_txl_block_bwd: null pointer");
    static bool attr = false;
    if (!attr) { if (int rc = block_lds((const void*)txl_block_bwd_kernel)) return rc; attr = true; }
    const int Q = block_share(d);
    const unsigned grid = Q == 1 ? (unsigned)d->B : (unsigned)((d->B + 7) / 8 * 8 * Q);
    txl_block_bwd_kernel<<<grid, 256, BLOCK_LDS, (hipStream_t)stream>>>(block_kernel_params(d, Q));
    return hulc_check_launch("hulc_txl_block_bwd");
}
