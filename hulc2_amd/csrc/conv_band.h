// conv_band.h — launch parameters shared by the LDS-band convolution kernels (conv_band.hip, conv_band_planes.hip), and what conv.hip
// asks the three band dispatchers for (conv_band.hip, conv1_band.hip, conv_wgrad_band.hip): declared here and nowhere else.
#pragma once
#include "hulc_common.h"
#include "hulc_abi_internal.h"

namespace hulc_band {

#define BAND_MAXCLS 4
struct BandCls {
    int OH, OW;                     // output grid of this weight set's class
    long y_off;                     // element offset of the class inside Y / mask (parity classes of a data gradient)
    int co_base;                    // first output channel of the set's 32-channel tile
    long w_row0;                    // first global weight row of the set
    long w_tap_off[16];             // global offset (elements, inside a weight row) of tap (ty, tx)
};
struct BandP {
    const void* X; void* Y; const void* Wt; const float* bias; const void* mask;
    const void* add;                // optional residual (bf16, laid out like Y), summed before the ReLU: the ResNet trunk's block outputs
    void* Y16;                      // optional (fp32 Y only): a bf16 copy of Y, same layout, from the same accumulators (hulc_conv_desc.y_bf16)
    int x_dtype, y_dtype, w_dtype, mask_dtype;
    int Nimg, H, W;                 // input tensor dims (NHWC, C = template)
    int OHmax, OWmax;               // largest class grid: defines the staged band
    int pad_y, pad_x;               // band origin: input row = oy*S + ty - pad_y
    int R;                          // output rows per work unit
    int F;                          // > 1: a work unit is F whole frames (small maps; then R == OHmax)
    long x_sn, x_sy, x_sx;          // input element strides
    long y_sn, y_sy, y_sx;          // output element strides (channels contiguous)
    long ldw;                       // global weight row stride (elements)
    int relu;
    unsigned* bits_out;             // optional: ReLU sign planes of Y (forward): dword (co / 32) * bplane + pixel, bit = channel % 32
    const unsigned* bits_in;        // optional: sign planes used as the mask (data gradient) instead of `mask`
    int bshift; long bplane;        // log2(channels of the tensor the planes describe), pixels of that tensor: planes are [channels / 32][pixels]
    BandCls cls[BAND_MAXCLS];
};
// One band launch as conv.hip requests it.  The caller fills p's operands, dtypes, Nimg / H / W, pads, strides, ldw, relu, planes and one cls
// entry per weight set (taps past TH * TW need not be set); the dispatcher derives R, F, OHmax, OWmax, bshift and bplane.
struct BandReq {
    int C, NSET, TH, TW, S;         // kernel instance: input channels, weight sets (= entries of p.cls), taps, input stride
    int bits_channels;              // channels of the tensor p.bits_out / p.bits_in describe
    BandP p;
    void drop_planes() { p.bits_out = nullptr; p.bits_in = nullptr; bits_channels = 0; }
};

// bf16 operands only (input band, weights, ReLU mask): a run-time dtype branch around a load makes hipcc wait for it at the join, which
// turned the 32+ weight-fragment loads of a launch and the 10+ chunk loads of every prefetch into as many serial memory round trips.
// Other storage types take the gather kernel in conv.hip.
HULC_DEVICE uint4 band_load_bits(const void* X, long off) { return *(const uint4*)((const uint16_t*)X + off); }
// XF32 instances (an fp32 gradient entering the gripper stack's conv3 data gradient): converted at load time, compile-time selected
template <bool XF32>
HULC_DEVICE uint4 band_load_x(const void* X, long off) {
    if (!XF32) return band_load_bits(X, off);
    const float4* q = (const float4*)((const float*)X + off);
    const float4 a = q[0], c = q[1];
    return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(c.x, c.y), pack_bf16x2(c.z, c.w));
}

// conv_band_planes.hip (direct-to-LDS loads into a chunk-major band, 64 input channels, the static camera's frame sizes): 0 = launched, -1 = not covered
int launch_band_planes(BandP& p, int NSET, int TH, int TW, hipStream_t s);

}  // namespace hulc_band

// The band dispatchers: 0 = launched, 1 = geometry not covered (the caller uses its gather kernel), < 0 = error (hulc_fail).
int hulc_conv_band_dispatch(const hulc_band::BandReq& rq, hipStream_t s);
// conv1 forward (NCHW fp32 or uint8 NHWC frames, 3 -> 32 channels, 8x8 stride 4); relu_bits: the planes this launch is to write, or null
int hulc_conv1_band_dispatch(const hulc_conv_desc& d, const float* x, const void* w, long ldw, const float* bias, void* y, unsigned* relu_bits, hipStream_t s);
// weight gradient; dw is [Cout][K] fp32 in the forward k order
int hulc_conv_wgrad_band_dispatch(const hulc_conv_desc& d, const void* x, const void* dy, float* dw, float* db, void* ws, long ws_bytes, hipStream_t s);

static inline int conv_OH(const hulc_conv_desc& d, int pad = 0) { return (d.H + 2 * pad - d.KH) / d.stride + 1; }
static inline int conv_OW(const hulc_conv_desc& d, int pad = 0) { return (d.W + 2 * pad - d.KW) / d.stride + 1; }

// conv1's frame sources, written into the kernel parameters P = C1P / W1P: frames n >= nsplit come from X2, pre-offset by -nsplit frames (X2 == x
// and nsplit == N without x2); xs / xs2: the optional device slots.  Returns which fields are unacceptable: the launchers word and order their refusals.
enum { CONV1_BAD_SLOTS = 1, CONV1_BAD_X2 = 2 };
template <typename P>
int conv1_frames(const hulc_conv_desc& d, const void* x, P& p) {
    const int u8 = d.x_u8_nhwc;
    int bad = 0;
    p.X2 = x; p.nsplit = d.N; p.xs = (const void* const*)d.x_slot; p.xs2 = (const void* const*)d.x2_slot;
    if ((d.x_slot || d.x2_slot) && (u8 || !d.x_slot || (d.x2_slot && !d.x2) || ((uintptr_t)d.x_slot | (uintptr_t)d.x2_slot) % 8)) bad |= CONV1_BAD_SLOTS;
    if (d.x2) {
        if (d.n_split < 0 || d.n_split > d.N || ((uintptr_t)d.x2 % (u8 ? 4 : 16)) || (u8 && d.frame_index)) return bad | CONV1_BAD_X2;
        p.X2 = (const char*)d.x2 - (long)d.n_split * 3 * d.H * d.W * (u8 ? 1 : 4);
        p.nsplit = d.n_split;
    }
    return bad;
}
