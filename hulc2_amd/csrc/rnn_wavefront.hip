// rnn_wavefront.hip — the 2-layer ReLU RNN of the action decoder as ONE persistent kernel per direction (bf16 compute).
//
// reference arithmetic: nn.RNN(num_layers=2, nonlinearity="relu", batch_first=True) of
// hulc2/models/decoders/logistic_decoder_rnn.py:70-79 (forward) and its autograd backward.
//
// The recurrence is latency-bound: per time step two skinny GEMMs (64 rows, K = 2048 / 4096) whose 25 MB of weights were
// re-streamed by ~130 launches per direction (12 us kernel + 4 us split-K epilogue each).  With
//     z_t = [h0_t | h1_{t-1}]  (one row block of the time-major state buffer)
// both layers advance together as a wavefront:     z_{t+1} = f( z_t W^T + add_t ),   W = [[W_hh0, 0], [W_ih1, W_hh1]]
// and the backward pass has the same shape on d_t = [delta1_t | delta0_{t+1}] with W = [[W_hh1^T, 0], [W_ih1^T, W_hh0^T]].
// So one kernel serves both directions:
//   * 256 workgroups (one per CU) = 2 row halves x H/16 column groups; a workgroup owns 16 "first" + 16 "second" output
//     columns for 32 batch rows and keeps its 16+16 weight columns (x K = 2H) in REGISTERS for all S+1 wave steps
//     (96 VGPRs per wave) — weights are read from HBM once per pass instead of once per step;
//   * per wave step a workgroup reads its 32 rows of the bf16 state copy (256 KB, from L2), runs v_mfma_f32_16x16x32_bf16
//     with the 8 waves splitting K, sums the 8 partial tiles through LDS in a fixed order (deterministic), applies the
//     epilogue (bias / external add / ReLU or stored-activation mask) and writes fp32 (for the weight-gradient GEMMs) and
//     bf16 (its own next operand, ping-pong) state;
//   * wave steps are separated by a device-wide barrier (agent-scope counters, one per row half and XCD).  All 256 workgroups
//     are co-resident (1 per CU by register footprint; the stream runs nothing else), the spin is bounded, and a timeout
//     poisons the output with NaN instead of hanging the GPU.
#include "hulc_common.h"
#include "hulc_abi_internal.h"
#include <type_traits>
#ifdef HULC_PROBES
#include <cstdio>
#include <stdlib.h>
#include <vector>
#endif

#define RNN_CTR_STRIDE 1024                                   // unsigned words between barrier counters (4 KB)
#define RNN_WS_HEADER (17 * RNN_CTR_STRIDE * 4)               // 16 barrier counters + the error word
#define RNN_ERR_WORD (16 * RNN_CTR_STRIDE)

namespace {

struct WaveP {
    float* z; long z_step;                       // fp32 state rows: wave step tau reads z + tau*z_step, writes z + (tau+1)*z_step
    uint16_t* zb;                                // bf16 mirror of the state rows, [S+2][B][2H] row-major (operand of the weight-gradient GEMMs)
    uint16_t* zt; long ld_t;                     // optional transposed mirror [2H][(S+2)*B] (token = region*B + row): k-major operand of the weight-gradient GEMMs
    uint16_t* xb;                                // the same values in the exchange layout the kernel itself reads, [S+2][2][H/8][64][8] (see below)
    int zb_row0, zb_dir;                         // region read at wave step tau = zb_row0 + tau * zb_dir (0, +1 forward; S+1, -1 reversed)
    const uint16_t *wA, *wB1, *wB2;              // first (H x H), second k < H (H x H), second k >= H (H x H)
    long ldA, ldB1, ldB2; int tA, tB1, tB2;      // t: element (n, k) is w[k*ld + n] instead of w[n*ld + k]
    const float* add1; long add1_step, ld_add1;  // per-step external term of the first half (nullable)
    const float *bias1a, *bias1b, *bias2a, *bias2b;
    const float* mask1; long mask1_step, ld_mask1;   // stored activations: output kept where mask > 0 (nullable)
    const float* mask2; long mask2_step, ld_mask2;
    int relu, S, B, H;
    unsigned* bar; int* err; int* err_sticky;
    const float* add1c; long ld_add1c;           // per-row constant of the first half, the same at every step (nullable): folded into the bias term
    int inject_timeout;                          // tests only (hulc_rnn_wave_desc.inject_timeout): the sweep ends as if a barrier had timed out
#ifdef HULC_PROBES
    unsigned long long* ts;                      // HULC_RNN_DBG & 8: s_memrealtime stamps [workgroup 0 / 100][wave 1, 0, 7][sub-step][7 phases] (printed by the next launch)
#endif
};

// The dropout instances (hulc_rnn_wavefront_drop) take the plain parameter block plus the mask's: the plain instances keep WaveP, so
// their argument block and their code are what they were.  The mask is never stored as values: element (t, row, j) is kept with scale
// 1 / (1 - p) when dropout_scale(seed ^ seed_dev[0], (t * B + row) * H + j, p) is non-zero, t = t0 + tau * t_dir at wave step tau.
struct WaveDropP : WaveP {
    float drop_p; unsigned long long seed; const unsigned long long* seed_dev;
    int t0, t_dir;
    const unsigned long long* keep;              // K-side mode: the keep BITS of the sweep in fragment order, written by rnn_keep_bits_kernel
};

// The paired instances (hulc_rnn_wavefront_pair) take the plain parameter block plus the second half's own external term and destinations: like
// the dropout instances they leave WaveP, and with it the plain and DROP instances, as they were.
struct WavePairP : WaveP {
    float* z2; long z2_step;                     // fp32 rows of the second half: wave step tau writes z2 + tau*z2_step, columns H .. 2H-1
    int zb2_row0, zb2_step;                      // bf16 mirror region of the second half at wave step tau = zb2_row0 + tau * zb2_step
    const float* add2; long add2_step, ld_add2;  // per-step external term of the second half (nullable)
    const float* add2c; long ld_add2c;           // per-row constant of the second half (nullable)
};

// The bf16 state copy is the only data exchanged between workgroups inside the kernel.  Measured alternatives:
//   * agent-scope release/acquire fences around the barrier: buffer_wbl2 / buffer_inv from 2048 waves per step, ~90 us/step;
//   * device-coherent (sc1) loads and stores on a ping-pong buffer: no cache maintenance, but every read bypasses the
//     per-XCD L2 -> 64 MB per step from memory, 14 us/step;
//   * (this) every wave step writes its OWN region of the copy with write-through sc1 stores and readers use ordinary
//     loads: a region's addresses are never cached before they are complete (first touch after the barrier; the caches
//     start clean at kernel launch), so the 128 workgroups sharing a row half hit the XCD's L2 instead of memory.
// Exchange layout: [region][state half][k / 8][row 0..63][8 values].  An MFMA A fragment is (row = lane % 16, 8 consecutive k
// at k-block lane / 16): in a row-major copy the 16 lanes of a k-block sit 8 KB apart, every lane is its own tag lookup and the
// 256 KB a workgroup reads per step took ~6 us (18 B/clk per CU).  Blocked, the 16 lanes read 256 contiguous bytes, an
// instruction touches 8 full lines instead of 64 partial ones, and every 128-byte line has exactly one writer workgroup.
HULC_DEVICE bf16x8_t load_state8(const uint16_t* p) { return *(const bf16x8_t*)p; }

// bit 0 / bit 1 of `two`: keep the low / high bf16 of w, else zero it.  hulc_common.h's keep_u16x2 does the same in one asm instruction, but
// the result here is the very next MFMA's A operand, and hipcc pads no VALU -> MFMA hazard behind an asm statement: plain C++
HULC_DEVICE uint32_t keep_pair(uint32_t w, uint32_t two) {
    const uint32_t lo = 0u - (two & 1u), hi = 0u - ((two >> 1) & 1u);
    return w & ((lo & 0xffffu) | (hi << 16));
}

// T: element (n, k) is w[k*ld + n] instead of w[n*ld + k] — compile-time, so that the 24 fragment loads of a wave are issued back to
// back (a run-time branch around a load makes hipcc wait for it at the join: 24 serial round trips at the start of every pass)
template <bool T>
HULC_DEVICE bf16x8_t load_w(const uint16_t* w, long ld, int n, int k) {
    union { uint4 u; bf16x8_t b; uint16_t h[8]; } x;
    if (!T) x.u = *(const uint4*)(w + (long)n * ld + k);
    else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x.h[j] = w[(long)(k + j) * ld + n];
    }
    return x.b;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// The sweep is software-pipelined over two independent row groups (round 3).
//
// An unpipelined wave step is a dependent chain: state loads + MFMA (2.8 us) -> 8-wave sum + epilogue -> write-through exchange stores ->
// their acknowledgement -> barrier arrival -> barrier propagation (1.3 us) -> next state loads: 6.5-7 us, the matrix pipes busy for 0.3 of them.
// Sequences (batch rows) are independent, so the 32 rows a workgroup owns are split into two groups of 16 (the two MFMA row tiles) with their OWN
// barrier counters, and the workgroup alternates between them: while group A's stores travel and its barrier collects the other workgroups,
// group B's state is fetched, multiplied and reduced.  Per sub-step roles (no wave waits for something it does not need):
//   wave 0      the exchange stores of the group just finished (64 lanes x 16 bytes = the whole 16 x 32 tile) and — one sub-step later, behind
//               the NEXT group's state loads — `s_waitcnt vmcnt(16)`: vector memory returns in order, so with 16 younger loads outstanding the
//               older stores have been acknowledged; then lane 0 bumps the group's barrier counter.  Nobody else waits for the acknowledgement.
//   waves 1-2   fp32 rows (read only after the kernel), wave 3 the row-major bf16 mirror, wave 4 the transposed mirror — from LDS tiles
//   wave 7      lanes 0-3 poll the four counters of (row half, group); it owns no stores, so its polling loads wait for nothing but themselves
//               (a polling load behind an un-acknowledged store would wait for that store first)
// Round 4, phase stamps (a -DHULC_PROBES build with HULC_RNN_DBG=8, the TS instance): a sub-step of 2.75 us = poll + barrier 0.3, state loads + MFMAs 1.35 (first wave) ... 1.85 (last
// wave: 128 KB per CU at 29 B/clk), 8-wave sum + epilogue 0.22, stores 0.13-0.23.  Reading the NEXT sub-step's counters at the end of this one (to save the
// round trip at the top) made the pass 11 % slower: the counters are not complete yet at that point — a group's chain (stores -> acknowledgement ->
// counter -> propagation -> loads -> MFMAs -> sum) is as long as the two sub-steps it has; the kernel is bound by that chain, not by throughput.
//
// DROP (hulc_rnn_wavefront_drop): inter-layer dropout on the second half's wB1 product, which then has an accumulator and a slice of the
// reduction tile of its own (the wB2 product and the first half read the same fragments undropped).
//   1, K side (forward sweep):  second = f2( s * ((keep . z[:, :H]) wB1^T) + z[:, H:] wB2^T + biases ): the dropped bf16 values of the A fragment
//      are zeroed (keep_pair) and s = 1 / (1 - p) multiplies the reduced product in fp32.  The keep bits are not drawn here (two draws per
//      fragment x 8 fragments per lane and sub-step at ~50 slots each, on the chain the kernel is bound by): a launch in front of the sweep
//      packs them so that a lane's 8 fragments of a sub-step are ONE 8-byte load, byte q = fragment q, bit j = its j-th value.
//   2, N side (backward sweep): second = f2( keep * s . (z[:, :H] wB1^T) + z[:, H:] wB2^T ): one draw per output element, taken beside the
//      epilogue operands while the state loads are in flight.
// Everything the workgroups exchange, wave 0's vmcnt constant included, is untouched: see the note at the keep-bit load.
//
// PAIR (hulc_rnn_wavefront_pair): the two halves are independent recurrences, z_{tau+1} = [ f1(z_tau[:, :H] wA^T + ..) | f2(z_tau[:, H:] wB2^T + ..) ],
// both written at every one of the S wave steps (no lag): the wB1 product is gone (no wfb registers, no MFMAs), the second tile reads af[1] only
// and has an external term of its own.  The exchange copy stays in sweep order (it is what the next wave step reads); the second half's fp32
// rows and row-major mirror rows go where WavePairP says.  PAIR == 2 is the solo sweep (wB2 == NULL): the second half is neither loaded,
// multiplied nor stored, so a sub-step has KPW state loads, and wave 0's vmcnt constant is NLD = the state loads of a sub-step in every mode.
template <int H, bool WT, bool TS = false, int DROP = 0, int PAIR = 0>      // TS: the probe's instance with phase time stamps (-DHULC_PROBES builds, HULC_RNN_DBG & 8) — the stamps' branches cost the plain kernel 5 %
__global__ __launch_bounds__(512) void rnn_wavefront2_kernel(std::conditional_t<PAIR != 0, WavePairP, std::conditional_t<DROP != 0, WaveDropP, WaveP>> p) {
    static_assert(PAIR == 0 || (DROP == 0 && !TS), "the paired sweep has no dropout and no probe instance");
    constexpr int NH = PAIR == 2 ? 1 : 2;        // state halves a sub-step loads
    constexpr int KS = H / 32;
    constexpr int KPW = KS / 8;
    constexpr int NLD = NH * KPW;                // state loads of a wave per sub-step
    constexpr int NR = DROP ? 3 : 2;             // reduction tiles: first half, second half, (DROP) the masked wB1 product
    static_assert(KS % 8 == 0, "H must be a multiple of 256");
    static_assert(DROP == 0 || KPW == 8, "the keep bits of a lane's sub-step are one 64-bit word: 8 fragments of 8 values");
    __shared__ float red[8][NR][256];            // [wave][ct][reg*64 + lane] partial tiles of the current group
    __shared__ uint4 wlds[8][KPW][64];
    __shared__ __attribute__((aligned(16))) uint16_t otile[16][2][16 + 8];   // bf16 outputs of the sub-step, [row][half][col] (+pad)
    __shared__ __attribute__((aligned(16))) float ftile[16][2][16 + 4];      // the same values in fp32
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, kb = lane >> 4;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int lgrp = xcd + 8 * (slot >> 2);
    const int rowhalf = lgrp & 1, n0 = ((lgrp >> 1) * 4 + (slot & 3)) * 16;
    const int nblk = gridDim.x;
    const long ldz = 2 * H;

    bf16x8_t wfa[KPW], wfb[KPW];
#pragma unroll
    for (int q = 0; q < KPW; ++q) {
        const int k = (wave * KPW + q) * 32 + kb * 8;
        wfa[q] = load_w<WT>(p.wA, p.ldA, n0 + i, k);
        if constexpr (PAIR == 0) wfb[q] = load_w<WT>(p.wB1, p.ldB1, n0 + i, k);
        if constexpr (PAIR != 2) {
            union { bf16x8_t b; uint4 u; } wc; wc.b = load_w<WT>(p.wB2, p.ldB2, n0 + i, k);
            wlds[wave][q][lane] = wc.u;
        }
    }
    // this thread's output of a sub-step: tile ct = tid >> 8, accumulator element e
    const int oct = tid >> 8, oe = tid & 255, oln = oe & 63;
    const int orow = 4 * (oln >> 4) + (oe >> 6);                  // row inside the 16-row group
    const int on = n0 + (oln & 15);
    float obias[2];                                               // per group (the per-row constant differs)
    {
        const float* ba = oct ? p.bias2a : p.bias1a;
        const float* bb = oct ? p.bias2b : p.bias1b;
        const float b0 = (ba ? ba[on] : 0.f) + (bb ? bb[on] : 0.f);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int m = rowhalf * 32 + g * 16 + orow;
            obias[g] = b0;
            if (!oct && p.add1c) obias[g] += p.add1c[(long)(m < p.B ? m : p.B - 1) * p.ld_add1c + on];
            if constexpr (PAIR == 1) { if (oct && p.add2c) obias[g] += p.add2c[(long)(m < p.B ? m : p.B - 1) * p.ld_add2c + on]; }
        }
    }
    int pending = -1;                                             // wave 0: group whose exchange stores await their acknowledgement
    const int NT = PAIR ? p.S : p.S + 1;                           // wave steps
    const int U = 2 * NT;
    unsigned long long dseed = 0ull; float dkeep = 1.f;           // (DROP) the call's RNG stream and 1 / (1 - p), as dropout_scale computes it
    if constexpr (DROP != 0) { dseed = p.seed ^ (p.seed_dev ? p.seed_dev[0] : 0ull); dkeep = 1.0f / (1.0f - p.drop_p); }
#ifdef HULC_PROBES
    // (probe) phase stamps of workgroups 0 and 100, waves 1 (an ordinary wave), 0 (exchange stores) and 7 (polls)
    const int ts_wg = blockIdx.x == 0 ? 0 : (blockIdx.x == 100 ? 1 : -1), ts_wv = wave == 1 ? 0 : (wave == 0 ? 1 : (wave == 7 ? 2 : -1));
    unsigned long long* ts = (TS && p.ts && ts_wg >= 0 && ts_wv >= 0 && lane == 0) ? p.ts + (long)((ts_wg * 3 + ts_wv) * 80) * 8 : nullptr;
#define RNN_TS(u_, ph_) if constexpr (TS) { if (ts && (u_) < 80) ts[(u_) * 8 + (ph_)] = __builtin_amdgcn_s_memrealtime(); }
#define RNN_TS_MFMA_DONE if constexpr (TS) { if (ts) __builtin_amdgcn_s_waitcnt(0xC07F); }   // (lgkmcnt(0): the partial tile is in LDS = the MFMAs are done)
#else
#define RNN_TS(u_, ph_)
#define RNN_TS_MFMA_DONE
#endif
    for (int u = 0; u < U; ++u) {
        const int g = u & 1, tau = u >> 1;
        RNN_TS(u, 0)
        const bool first_on = PAIR ? true : tau < p.S, second_on = PAIR ? PAIR == 1 : tau >= 1;
        const int om = rowhalf * 32 + g * 16 + orow;
        if (tau > 0) {
            // ---- inputs of (g, tau): every workgroup of this row half has published the group's z_tau
            if (wave == 7 && lane < 4) {
                const unsigned per = (unsigned)(nblk / 8) * (unsigned)tau;
                const unsigned* bar = p.bar + (g * 8 + (xcd & 1) + 2 * lane) * RNN_CTR_STRIDE;
                long spins = 0;
                while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < per) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1L << 22)) {
                        __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (p.err_sticky) __hip_atomic_fetch_or(p.err_sticky, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
            }
            __syncthreads();
            asm volatile("" ::: "memory");
        }
        RNN_TS(u, 1)
        f32x4_t acc[NR];
#pragma unroll
        for (int ct = 0; ct < NR; ++ct) acc[ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const bool mul = tau > 0;
        bf16x8_t af[2][KPW];
        if (mul) {
            const uint16_t* a = p.xb + (long)(p.zb_row0 + tau * p.zb_dir) * 64 * ldz + (long)(rowhalf * 32 + g * 16 + i) * 8;
#pragma unroll
            for (int hf = 0; hf < NH; ++hf)
#pragma unroll
                for (int q = 0; q < KPW; ++q) af[hf][q] = load_state8(a + ((long)(hf * (H / 8) + (wave * KPW + q) * 4 + kb) * 64) * 8);
        }
        if (wave == 0 && pending >= 0) {
            // the previous sub-step's exchange stores are OLDER than everything this wave has issued since (compiler barrier after them): once at
            // most the NLD (2 * KPW; solo sweep: KPW) state loads above are outstanding they have been acknowledged — the other workgroups may read them
            asm volatile("" ::: "memory");
            if (mul) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLD) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_fetch_add(p.bar + (pending * 8 + xcd) * RNN_CTR_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pending = -1;
        }
        // epilogue operands: requested behind the state loads (their latency hides under the MFMAs) and consumed as opaque values in the
        // epilogue — hipcc otherwise hoists the `mask > 0` compare to the load and waits for it (and for everything older) right here
        float oadd = 0.f, omask = 1.f;
        {
            const int m = om < p.B ? om : p.B - 1;
            if (oct == 0) {
                if (p.add1 && first_on) oadd = p.add1[(long)tau * p.add1_step + (long)m * p.ld_add1 + on];
                if (p.mask1 && first_on) omask = p.mask1[(long)tau * p.mask1_step + (long)m * p.ld_mask1 + on];
            } else {
                if constexpr (PAIR == 1) { if (p.add2) oadd = p.add2[(long)tau * p.add2_step + (long)m * p.ld_add2 + on]; }
                if (p.mask2 && second_on) omask = p.mask2[(long)tau * p.mask2_step + (long)m * p.ld_mask2 + on];
            }
        }
        // (DROP) the mask of this sub-step.  K side: this lane's 64 keep bits — a vector load issued HERE, behind wave 0's wait like the
        // epilogue operands above (the "memory" clobbers of that block keep it below): between the exchange stores and the wait wave 0 still
        // issues the 2 * KPW state loads and nothing else, so vmcnt(2 * KPW) proves the stores acknowledged exactly as in the plain kernel.
        // The words were written by the launch in front of the sweep; no workgroup writes them.  N side: the scale of this thread's output.
        unsigned long long kbits = 0ull; float oscale = 0.f;
        if constexpr (DROP == 1) {
            if (mul) kbits = p.keep[((long)((p.t0 + tau * p.t_dir) * 8 + wave) * 4 + kb) * 64 + rowhalf * 32 + g * 16 + i];
        } else if constexpr (DROP == 2) {
            if (oct == 1 && second_on) {
                const int m = om < p.B ? om : p.B - 1;
                oscale = dropout_scale(dseed, (uint64_t)((long)(p.t0 + tau * p.t_dir) * p.B + m) * (uint64_t)H + (uint64_t)on, p.drop_p);
            }
        }
        if (mul) {
            if constexpr (PAIR != 0) {
#pragma unroll
                for (int q = 0; q < KPW; ++q) acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfa[q], acc[0], 0, 0, 0);
            } else if constexpr (DROP == 0) {
#pragma unroll
                for (int q = 0; q < KPW; ++q) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfa[q], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfb[q], acc[1], 0, 0, 0);
                }
            } else if constexpr (DROP == 2) {
#pragma unroll
                for (int q = 0; q < KPW; ++q) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfa[q], acc[0], 0, 0, 0);
                    acc[NR - 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfb[q], acc[NR - 1], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int q = 0; q < KPW; ++q) acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][q], wfa[q], acc[0], 0, 0, 0);
            }
            if constexpr (PAIR != 2) {
#pragma unroll
                for (int q = 0; q < KPW; ++q) {
                    union { bf16x8_t b; uint4 u; } wc; wc.u = wlds[wave][q][lane];
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][q], wc.b, acc[1], 0, 0, 0);
                }
            }
            if constexpr (DROP == 1) {
                // the masked product last: the keep bits were requested after the state loads
                const unsigned klo = (unsigned)kbits, khi = (unsigned)(kbits >> 32);
#pragma unroll
                for (int q = 0; q < KPW; ++q) {
                    const unsigned k8 = ((q < 4 ? klo : khi) >> (8 * (q & 3))) & 0xffu;
                    union { bf16x8_t b; uint4 u; } a; a.b = af[0][q];
                    a.u.x = keep_pair(a.u.x, k8); a.u.y = keep_pair(a.u.y, k8 >> 2);
                    a.u.z = keep_pair(a.u.z, k8 >> 4); a.u.w = keep_pair(a.u.w, k8 >> 6);
                    acc[NR - 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.b, wfb[q], acc[NR - 1], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < NR; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave][ct][e * 64 + lane] = acc[ct][e];
        RNN_TS_MFMA_DONE
        RNN_TS(u, 2)
        __syncthreads();
        RNN_TS(u, 3)
        // ---- fixed-order sum over the 8 K slices + epilogue: 512 outputs, one per thread
        {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) v += red[w][oct][oe];
            if constexpr (DROP != 0) {
                if (oct == 1) {                                    // + scale * the masked wB1 product, summed in the same fixed order
                    float vd = 0.f;
#pragma unroll
                    for (int w = 0; w < 8; ++w) vd += red[w][NR - 1][oe];
                    v += (DROP == 1 ? dkeep : oscale) * vd;
                }
            }
            const bool on_ = oct == 0 ? first_on : second_on;
            asm volatile("" : "+v"(oadd), "+v"(omask));
            v += oadd + obias[g];
            if ((oct == 0 ? p.mask1 : p.mask2) != nullptr) v = omask > 0.f ? v : 0.f;
            else if (p.relu) v = fmaxf(v, 0.f);
            if (!on_) v = 0.f;
            otile[orow][oct][on - n0] = f32_to_bf16_bits(v);
            ftile[orow][oct][on - n0] = v;
        }
        RNN_TS(u, 4)
        __syncthreads();
        RNN_TS(u, 5)
        const int region = p.zb_row0 + (tau + 1) * p.zb_dir;
        // which halves of this sub-step are stored (plain: the first half while it is on, the second always, zero at tau = 0; paired: both; solo: the first)
        auto stored = [&](int ct) { return PAIR ? (ct == 0 || PAIR == 1) : (ct == 1 || first_on); };
        if (wave == 0) {
            // exchange copy: lane = (row 0..15, half, 8-column chunk); skipped once nobody reads it any more (last wave step)
            const int row = lane & 15, ct = (lane >> 4) & 1, ch = lane >> 5;
            const int m = rowhalf * 32 + g * 16 + row;
            if (PAIR ? tau + 1 < p.S : tau < p.S) {
                if (m < p.B && stored(ct)) {
                    const uint4 v16 = *(const uint4*)&otile[row][ct][ch * 8];
                    unsigned long long* dst = (unsigned long long*)(p.xb + (long)region * 64 * ldz + ((long)(ct * (H / 8) + n0 / 8 + ch) * 64 + m) * 8);
                    __hip_atomic_store(dst, (unsigned long long)v16.x | ((unsigned long long)v16.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(dst + 1, (unsigned long long)v16.z | ((unsigned long long)v16.w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                pending = g;
            }
            asm volatile("" ::: "memory");                         // nothing this wave loads later may be hoisted above the stores
        } else if (wave <= 2) {
            // fp32 rows: 16 rows x 2 halves x 4 chunks of 4 columns = 128 float4 pieces
            const int t = tid - 64, row = t & 15, ct = (t >> 4) & 1, ch = t >> 5;
            const int m = rowhalf * 32 + g * 16 + row;
            if (m < p.B && stored(ct)) {
                float* zn = p.z + (long)(tau + 1) * p.z_step;
                if constexpr (PAIR == 1) { if (ct) zn = p.z2 + (long)tau * p.z2_step; }
                *(float4*)(zn + (long)m * ldz + ct * H + n0 + ch * 4) = *(const float4*)&ftile[row][ct][ch * 4];
            }
        } else if (wave == 3) {
            const int row = lane & 15, ct = (lane >> 4) & 1, ch = lane >> 5;
            const int m = rowhalf * 32 + g * 16 + row;
            int rg = region;
            if constexpr (PAIR == 1) { if (ct) rg = p.zb2_row0 + tau * p.zb2_step; }
            if (m < p.B && stored(ct))
                *(uint4*)(p.zb + (long)rg * p.B * ldz + (long)m * ldz + ct * H + n0 + ch * 8) = *(const uint4*)&otile[row][ct][ch * 8];
        } else if (wave == 4 && p.zt) {
            // transposed mirror: lane = (half, column, 8-row chunk)
            const int ct = lane >> 5, col = (lane >> 1) & 15, ch = lane & 1;
            const int m = rowhalf * 32 + g * 16 + ch * 8;
            if (m < p.B && stored(ct)) {                          // B % 8 == 0 (checked by the launcher); the paired launcher hands in no transposed mirror
                unsigned w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = (unsigned)otile[ch * 8 + 2 * e][ct][col] | ((unsigned)otile[ch * 8 + 2 * e + 1][ct][col] << 16);
                *(uint4*)(p.zt + (long)(ct * H + n0 + col) * p.ld_t + (long)region * p.B + m) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        // (the LDS tiles are rewritten two barriers later: no extra barrier needed here)
        RNN_TS(u, 6)
    }
#undef RNN_TS
#undef RNN_TS_MFMA_DONE
    __syncthreads();
    if (p.inject_timeout && blockIdx.x == 0 && tid == 0) {
        __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p.err_sticky) __hip_atomic_fetch_or(p.err_sticky, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        // the last row each half wrote (plain: row S+1, whose first half is never produced)
        float* zn = p.z + (long)(PAIR ? p.S : p.S + 1) * p.z_step;
        float* zn2 = zn;
        if constexpr (PAIR == 1) zn2 = p.z2 + (long)(p.S - 1) * p.z2_step;
        for (int o = tid; o < 32 * 16; o += 512) {
            const int m = rowhalf * 32 + o / 16, n = n0 + o % 16;
            if (m < p.B) { zn[(long)m * ldz + n] = __builtin_nanf(""); if (PAIR != 2) zn2[(long)m * ldz + H + n] = __builtin_nanf(""); }
        }
    }
}

// zero the barrier header and the bf16 mirror of the initial state row: a kernel, not hipMemsetAsync, so that a captured hipGraph holds
// nothing but kernel nodes with plain pointer arguments (a captured hipMemsetAsync node
// was found to leave the barrier header un-zeroed on later replays once other allocations ran in between: NaN from replay 2 on, round 2)
__global__ __launch_bounds__(256) void rnn_prep_kernel(uint4* __restrict__ a, long na, uint4* __restrict__ b, long nb, float4* __restrict__ z0, long nz0,
                                                       float* __restrict__ zl, int B, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    if (i < na) a[i] = z;
    if (i < nb) b[i] = z;
    // the fp32 state rows the sweep reads but never writes: the initial row (B x 2H) and the FIRST half of the last row (its second half is
    // the sweep's final output) — were four torch fill launches per step
    if (z0 && i < nz0) z0[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (zl && i < (long)B * H / 4) { const long e = i * 4; *(float4*)(zl + (e / H) * 2 * H + e % H) = make_float4(0.f, 0.f, 0.f, 0.f); }
}

// rows x width bf16 elements at row pitch `pitch` <- 0 (initial-state column block of the transposed mirror)
__global__ __launch_bounds__(256) void rnn_zero2d_kernel(uint16_t* __restrict__ dst, long pitch, int width, int rows) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)rows * width) dst[(i / width) * pitch + i % width] = 0;
}

// The keep bits of a K-side sweep, [t][wave 0..7][k-block 0..3][row 0..63] 64-bit words: byte q of a word = the fragment q of that lane, i.e. the
// 8 values k = (wave * 8 + q) * 32 + kb * 8 .. + 7 of (t, row); bit j set = value j kept.  One thread per byte, two dropout_scale4 draws: the bits are
// those of dropout_scale(seed, (t * B + row) * H + k, p).  Rows >= B (never stored by the sweep) get zeros.
template <int H>
__global__ __launch_bounds__(256) void rnn_keep_bits_kernel(unsigned char* __restrict__ bits, int S, int B, float p, unsigned long long seed,
                                                            const unsigned long long* __restrict__ seed_dev) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)S * 8 * 4 * 64 * 8) return;
    if (seed_dev) seed ^= seed_dev[0];
    const int q = (int)(i & 7), row = (int)((i >> 3) & 63), kb = (int)((i >> 9) & 3), wave = (int)((i >> 11) & 7);
    const long t = i >> 14;
    unsigned b = 0;
    if (row < B) {
        const uint64_t idx = (uint64_t)(t * B + row) * (uint64_t)H + (uint64_t)((wave * 8 + q) * 32 + kb * 8);
        float s[4];
        dropout_scale4(seed, idx, p, s);
        b = (s[0] > 0.f ? 1u : 0u) | (s[1] > 0.f ? 2u : 0u) | (s[2] > 0.f ? 4u : 0u) | (s[3] > 0.f ? 8u : 0u);
        dropout_scale4(seed, idx + 4, p, s);
        b |= (s[0] > 0.f ? 16u : 0u) | (s[1] > 0.f ? 32u : 0u) | (s[2] > 0.f ? 64u : 0u) | (s[3] > 0.f ? 128u : 0u);
    }
    bits[i] = (unsigned char)b;
}

// out[r][j .. j+3] = x[r * ldx + j ..] * dropout_scale(seed, (row0 + r) * H + j .., p): four consecutive elements share one draw (H % 4 == 0)
__global__ __launch_bounds__(256) void rnn_drop_rows_kernel(const float* __restrict__ x, long ldx, long rows, int H, long row0, float p,
                                                            unsigned long long seed, const unsigned long long* __restrict__ seed_dev,
                                                            float* __restrict__ out32, long ld32, uint16_t* __restrict__ out16, long ld16) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H4 = H / 4;
    if (i >= rows * H4) return;
    if (seed_dev) seed ^= seed_dev[0];
    const long r = i / H4; const int j = (int)(i % H4) * 4;
    float s[4];
    dropout_scale4(seed, (uint64_t)(row0 + r) * (uint64_t)H + (uint64_t)j, p, s);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = x[r * ldx + j + e] * s[e];
        if (out32) out32[r * ld32 + j + e] = v;
        if (out16) out16[r * ld16 + j + e] = f32_to_bf16_bits(v);
    }
}

}  // namespace

extern "C" long hulc_rnn_wavefront_mirror_offset(void) { return RNN_WS_HEADER; }
// header | row-major mirror | exchange copy | transposed mirror (2H, (S+2)*B) when B % 8 == 0
extern "C" long hulc_rnn_wavefront_mirror_t_offset(int S, int B, int H) { return B % 8 ? 0 : RNN_WS_HEADER + (long)(S + 2) * (B + 64) * 2 * H * 2; }
extern "C" long hulc_rnn_wavefront_workspace(int S, int B, int H) { return RNN_WS_HEADER + (long)(S + 2) * (B + 64 + (B % 8 ? 0 : B)) * 2 * H * 2; }

// the refusals of a sweep, all of them before the first launch: a refused call writes nothing.  0 = the call may go ahead.  One list for
// every entry point: `pair` (hulc_rnn_wavefront_pair) takes no wB1 (pointer, pitch and layout flag are ignored) and an optional wB2
#define WAVE_FAIL(code, text) return hulc_fail(code, pair ? "hulc_rnn_wavefront_pair: " text : "hulc_rnn_wavefront: " text)
static int wave_refusal(const hulc_rnn_wave_desc* d, void* ws, bool pair = false) {
    if (!d || !ws || !d->z || !d->wA || (!pair && (!d->wB1 || !d->wB2))) WAVE_FAIL(-1, "null pointer");
    const bool hasB1 = !pair, hasB2 = d->wB2 != nullptr;
    if (d->H != 2048) WAVE_FAIL(-2, "built for hidden size 2048 (use the per-step hulc_gemm path otherwise)");
    if (d->B < 1 || d->B > 64 || d->S < 1) WAVE_FAIL(-2, "needs 1 <= B <= 64 rows and S >= 1");
    if ((!d->tA && (d->ldA % 8 || (uintptr_t)d->wA % 16)) || (hasB1 && !d->tB1 && (d->ldB1 % 8 || (uintptr_t)d->wB1 % 16)) ||
        (hasB2 && !d->tB2 && (d->ldB2 % 8 || (uintptr_t)d->wB2 % 16)))
        WAVE_FAIL(-4, "k-major weights must be 16-byte aligned");
    if ((hasB1 && d->tA != d->tB1) || (hasB2 && d->tA != d->tB2)) {
        if (pair) return hulc_fail(-3, "hulc_rnn_wavefront_pair: the two weight matrices share one layout (tA == tB2)");
        return hulc_fail(-3, "hulc_rnn_wavefront: the three weight matrices share one layout (tA == tB1 == tB2)");
    }
    if ((uintptr_t)ws % 16 || RNN_WS_HEADER % 16) WAVE_FAIL(-4, "workspace must be 16-byte aligned");
    return 0;
}
#undef WAVE_FAIL

// the kernel's parameter block of an accepted call
static void wave_params(const hulc_rnn_wave_desc* d, void* ws, WaveP& p) {
    p.z = d->z; p.z_step = d->z_step;
    p.bar = (unsigned*)ws; p.err = (int*)((unsigned*)ws + RNN_ERR_WORD); p.zb = (uint16_t*)((char*)ws + RNN_WS_HEADER);
    p.xb = p.zb + (long)(d->S + 2) * d->B * 2 * d->H;
    p.zt = (d->B % 8 || !d->mirror_t) ? nullptr : (uint16_t*)((char*)ws + hulc_rnn_wavefront_mirror_t_offset(d->S, d->B, d->H));
    p.ld_t = (long)(d->S + 2) * d->B;
    p.wA = (const uint16_t*)d->wA; p.wB1 = (const uint16_t*)d->wB1; p.wB2 = (const uint16_t*)d->wB2;
    p.ldA = d->ldA; p.ldB1 = d->ldB1; p.ldB2 = d->ldB2; p.tA = d->tA; p.tB1 = d->tB1; p.tB2 = d->tB2;
    p.add1 = d->add1; p.add1_step = d->add1_step; p.ld_add1 = d->ld_add1;
    p.bias1a = d->bias1a; p.bias1b = d->bias1b; p.bias2a = d->bias2a; p.bias2b = d->bias2b;
    p.mask1 = d->mask1; p.mask1_step = d->mask1_step; p.ld_mask1 = d->ld_mask1;
    p.mask2 = d->mask2; p.mask2_step = d->mask2_step; p.ld_mask2 = d->ld_mask2;
    p.relu = d->relu; p.S = d->S; p.B = d->B; p.H = d->H; p.err_sticky = d->err_sticky;
    p.add1c = d->add1c; p.ld_add1c = d->ld_add1c;
    p.inject_timeout = d->inject_timeout;
    p.zb_row0 = d->z_step > 0 ? 0 : d->S + 1; p.zb_dir = d->z_step > 0 ? 1 : -1;
#ifdef HULC_PROBES
    p.ts = nullptr;
#endif
}

// the launches in front of the sweep: barrier words, and the bf16 copy of the (zero) initial state row — the copy is a full mirror of the
// fp32 rows for the weight-gradient GEMMs
static void wave_prep(const hulc_rnn_wave_desc* d, void* ws, const WaveP& p, hipStream_t s) {
    const long na = RNN_WS_HEADER / 16, nb = (long)d->B * 2 * d->H * 2 / 16;
    const long nz0 = d->zero_edges ? (long)d->B * 2 * d->H / 4 : 0;
    long n = na > nb ? na : nb;
    if (nz0 > n) n = nz0;
    float* zlast = d->zero_edges ? d->z + (long)(d->S + 1) * d->z_step : nullptr;       // row S+1 of the sweep
    rnn_prep_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((uint4*)ws, na, (uint4*)(p.zb + (long)p.zb_row0 * d->B * 2 * d->H), nb,
                                                              d->zero_edges ? (float4*)d->z : nullptr, nz0, zlast, d->B, d->H);
    if (p.zt) {
        const long n = 2L * d->H * d->B;
        rnn_zero2d_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(p.zt + (long)p.zb_row0 * d->B, p.ld_t, d->B, 2 * d->H);
    }
}

// see include/hulc2_amd.h
extern "C" int hulc_rnn_wavefront(const hulc_rnn_wave_desc* d, void* ws, void* stream) {
    if (const int rc = wave_refusal(d, ws)) return rc;
    hipStream_t s = (hipStream_t)stream;
    WaveP p;
    wave_params(d, ws, p);
#ifdef HULC_PROBES
    if (getenv("HULC_RNN_DBG") && (atoi(getenv("HULC_RNN_DBG")) & 8)) {                                   // (probe, eager launches only: the next call prints the previous launch's phase stamps)
        static unsigned long long* buf = nullptr; static int calls = 0;
        const int NW = 2 * 3 * 80 * 8;
        if (!buf) { hipMalloc(&buf, NW * 8); hipMemset(buf, 0, NW * 8); }
        if (calls >= 1 && calls <= 4) {
            std::vector<unsigned long long> h(NW);
            hipMemcpy(h.data(), buf, NW * 8, hipMemcpyDeviceToHost);
            const char* wn[3] = {"wave 1", "wave 0 (exchange)", "wave 7 (poll)"};
            for (int wg = 0; wg < 2; ++wg) for (int wv = 0; wv < 3; ++wv) {
                double ph[7] = {0, 0, 0, 0, 0, 0, 0}; int cnt = 0;
                for (int u = 8; u < 60; ++u) {
                    const unsigned long long* t = &h[((wg * 3 + wv) * 80 + u) * 8];
                    const unsigned long long* tn = t + 8;
                    if (!t[0] || !tn[0]) continue;
                    for (int k = 0; k < 6; ++k) ph[k] += (double)(t[k + 1] - t[k]);
                    ph[6] += (double)(tn[0] - t[6]); ++cnt;
                }
                if (cnt) fprintf(stderr, "[rnn stamps call %d wg %d %s, 10 ns ticks, mean of %d sub-steps] poll+sync %.1f | loads+mfma %.1f | sync2 %.1f | sum+epilogue %.1f | sync3 %.1f | stores %.1f | loop %.1f\n",
                                 calls - 1, wg ? 100 : 0, wn[wv], cnt, ph[0] / cnt, ph[1] / cnt, ph[2] / cnt, ph[3] / cnt, ph[4] / cnt, ph[5] / cnt, ph[6] / cnt);
            }
        }
        if (calls < 4) p.ts = buf;
        ++calls;
    }
#endif
    wave_prep(d, ws, p, s);
#ifdef HULC_PROBES
    if (p.ts) {
        if (d->tA) rnn_wavefront2_kernel<2048, true, true><<<2 * (2048 / 16), 512, 0, s>>>(p);
        else rnn_wavefront2_kernel<2048, false, true><<<2 * (2048 / 16), 512, 0, s>>>(p);
    } else
#endif
    if (d->tA) rnn_wavefront2_kernel<2048, true><<<2 * (2048 / 16), 512, 0, s>>>(p);
    else rnn_wavefront2_kernel<2048, false><<<2 * (2048 / 16), 512, 0, s>>>(p);
    return hulc_check_launch("hulc_rnn_wavefront");
}

// the plain workspace, then the keep bits of a K-side sweep (S x 2048 words of 8 bytes at H = 2048)
static long wave_keep_offset(int S, int B, int H) { return (hulc_rnn_wavefront_workspace(S, B, H) + 15) / 16 * 16; }
extern "C" long hulc_rnn_wavefront_drop_workspace(int S, int B, int H) { return wave_keep_offset(S, B, H) + (long)S * 8 * 4 * 64 * 8; }

// see include/hulc2_amd.h
extern "C" int hulc_rnn_wavefront_drop(const hulc_rnn_wave_desc* d, float drop_p, unsigned long long seed, const unsigned long long* seed_dev,
                                       int mode, int t0, int t_dir, void* ws, void* stream) {
    if (!(drop_p >= 0.f) || !(drop_p < 1.f)) return hulc_fail(-2, "hulc_rnn_wavefront_drop: drop_p must be in [0, 1)");
    if (drop_p == 0.f) return hulc_rnn_wavefront(d, ws, stream);                    // no mask: the plain sweep, launch for launch
    if (const int rc = wave_refusal(d, ws)) return rc;
    if (mode != HULC_RNN_DROP_K && mode != HULC_RNN_DROP_N)
        return hulc_fail(-2, "hulc_rnn_wavefront_drop: mode is HULC_RNN_DROP_K or HULC_RNN_DROP_N");
    // the masked product exists at wave steps 1 .. S: their time indices must be those of the S x B x H mask
    const long ta = (long)t0 + t_dir, tb = (long)t0 + (long)d->S * t_dir;
    if ((t_dir != 1 && t_dir != -1) || ta < 0 || ta >= d->S || tb < 0 || tb >= d->S)
        return hulc_fail(-2, "hulc_rnn_wavefront_drop: t0 + tau * t_dir must stay in 0 .. S-1 for tau = 1 .. S (t_dir = +1 or -1)");
    hipStream_t s = (hipStream_t)stream;
    WaveDropP p;
    wave_params(d, ws, p);
    p.drop_p = drop_p; p.seed = seed; p.seed_dev = seed_dev; p.t0 = t0; p.t_dir = t_dir;
    p.keep = (const unsigned long long*)((char*)ws + wave_keep_offset(d->S, d->B, d->H));
    wave_prep(d, ws, p, s);
    if (mode == HULC_RNN_DROP_K) {
        const long n = (long)d->S * 8 * 4 * 64 * 8;
        rnn_keep_bits_kernel<2048><<<(unsigned)((n + 255) / 256), 256, 0, s>>>((unsigned char*)p.keep, d->S, d->B, p.drop_p, p.seed, p.seed_dev);
        if (d->tA) rnn_wavefront2_kernel<2048, true, false, 1><<<2 * (2048 / 16), 512, 0, s>>>(p);
        else rnn_wavefront2_kernel<2048, false, false, 1><<<2 * (2048 / 16), 512, 0, s>>>(p);
    } else {
        if (d->tA) rnn_wavefront2_kernel<2048, true, false, 2><<<2 * (2048 / 16), 512, 0, s>>>(p);
        else rnn_wavefront2_kernel<2048, false, false, 2><<<2 * (2048 / 16), 512, 0, s>>>(p);
    }
    return hulc_check_launch("hulc_rnn_wavefront_drop");
}

// see include/hulc2_amd.h
extern "C" int hulc_rnn_wavefront_pair(const hulc_rnn_wave_desc* d, float* z2, long z2_step, int mirror_row0, int mirror_step, const float* add2,
                                       long add2_step, long ld_add2, const float* add2c, long ld_add2c, void* ws, void* stream) {
    // the refusals, all of them before the first launch: the sweeps' common list, then this entry's own
    if (const int rc = wave_refusal(d, ws, true)) return rc;
    const bool solo = d->wB2 == nullptr;
    if (d->mirror_t) return hulc_fail(-2, "hulc_rnn_wavefront_pair: no transposed mirror (mirror_t must be 0)");
    if (!solo) {
        if (!z2) return hulc_fail(-1, "hulc_rnn_wavefront_pair: null pointer (z2)");
        const long ra = mirror_row0, rb = (long)mirror_row0 + (long)(d->S - 1) * mirror_step;
        if (ra < 0 || ra > d->S + 1 || rb < 0 || rb > d->S + 1)
            return hulc_fail(-2, "hulc_rnn_wavefront_pair: mirror_row0 + tau * mirror_step must stay in 0 .. S+1 for tau = 0 .. S-1");
    }
    hipStream_t s = (hipStream_t)stream;
    WavePairP p;
    wave_params(d, ws, p);
    p.wB1 = nullptr; p.zt = nullptr;
    p.z2 = z2; p.z2_step = z2_step; p.zb2_row0 = mirror_row0; p.zb2_step = mirror_step;
    p.add2 = add2; p.add2_step = add2_step; p.ld_add2 = ld_add2; p.add2c = add2c; p.ld_add2c = ld_add2c;
    // the launch in front of the sweep: barrier words, the mirror's initial region and (zero_edges) the fp32 row at d->z
    const long na = RNN_WS_HEADER / 16, nb = (long)d->B * 2 * d->H * 2 / 16, nz0 = d->zero_edges ? (long)d->B * 2 * d->H / 4 : 0;
    const long n = na > nb ? (na > nz0 ? na : nz0) : (nb > nz0 ? nb : nz0);
    rnn_prep_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((uint4*)ws, na, (uint4*)(p.zb + (long)p.zb_row0 * d->B * 2 * d->H), nb,
                                                              d->zero_edges ? (float4*)d->z : nullptr, nz0, nullptr, d->B, d->H);
    if (solo) {
        if (d->tA) rnn_wavefront2_kernel<2048, true, false, 0, 2><<<2 * (2048 / 16), 512, 0, s>>>(p);
        else rnn_wavefront2_kernel<2048, false, false, 0, 2><<<2 * (2048 / 16), 512, 0, s>>>(p);
    } else {
        if (d->tA) rnn_wavefront2_kernel<2048, true, false, 0, 1><<<2 * (2048 / 16), 512, 0, s>>>(p);
        else rnn_wavefront2_kernel<2048, false, false, 0, 1><<<2 * (2048 / 16), 512, 0, s>>>(p);
    }
    return hulc_check_launch("hulc_rnn_wavefront_pair");
}

// see include/hulc2_amd.h
extern "C" int hulc_rnn_drop_rows(const float* x, long ldx, long rows, int H, long row0, float drop_p, unsigned long long seed,
                                  const unsigned long long* seed_dev, float* out32, long ld32, void* out16, long ld16, void* stream) {
    if (rows == 0) return 0;
    if (!x || (!out32 && !out16)) return hulc_fail(-1, "hulc_rnn_drop_rows: null pointer");
    if (rows < 0 || H < 4 || H % 4 || row0 < 0 || ldx < H || (out32 && ld32 < H) || (out16 && ld16 < H))
        return hulc_fail(-2, "hulc_rnn_drop_rows: needs rows >= 0, H a positive multiple of 4, row0 >= 0 and pitches >= H");
    if (!(drop_p >= 0.f) || !(drop_p < 1.f)) return hulc_fail(-2, "hulc_rnn_drop_rows: drop_p must be in [0, 1)");
    const long n = rows * (H / 4);
    rnn_drop_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, ldx, rows, H, row0, drop_p, seed, seed_dev, out32, ld32,
                                                                                     (uint16_t*)out16, ld16);
    return hulc_check_launch("hulc_rnn_drop_rows");
}
