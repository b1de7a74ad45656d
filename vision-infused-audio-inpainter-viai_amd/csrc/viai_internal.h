// Internal (non-ABI) declarations shared between the kernel translation units.
#pragma once
#include "viai_common.h"
#include "../../include/viai_hip.h"

struct ConvArgs {
    const float* in;      // gathered NHWC tensor, channels [0, C1)
    const float* in2;     // optional second source, channels [C1, C1+C2) (virtual concat)
    const float* wp;      // packed weights [Cout][wtaps][C1+C2]
    const float* bias;    // [Cout] or null
    float* out;           // NHWC, channels [0, OC1)
    float* out2;          // optional second destination, channels [OC1, Cout)
    float* stat;          // optional BN partials [2][Cout][nblk_m]
    int C1, C2, Cout, OC1;
    int M, nblk_m, nblk_n;
    int act;              // fused activation (only when stat == null)
    float slope;
    int wfrag;            // WLayout of wp (split-precision kernels)
    const float* amax;    // f16x2 launches: device scalar max |gathered tensor| (dynamic operand scale, data gradients); null = static F16_ASCALE
    int in_p16;           // 1: the gathered tensor (in; no in2) is stored pre-split (P16 planes, viai_bf3.h) with the scale of *amax
    ConvGeom g;
};

struct WgradArgs {
    const float* x; const float* x2;   // forward input (virtual concat C1 + C2)
    const float* dy;                   // [M][Cout]
    float* ws;                         // [ksplit][wtaps][Cout][Cin]
    const float* amax;                 // f16x2 launch: device scalar max |dy| (dynamic operand scale); null = bf16x3
    const float* xmax;                 // f16x2 launch: device scalar max |x| (and |x2|) if known (dynamic operand scale for the forward input); null = static F16_ASCALE
    int C1, C2, Cout;
    int M;
    int nblk_co, nblk_ci, ksplit, chunks_per_split;
    int dy_p16, x_p16;                 // 1: dy / x (no x2) stored pre-split (P16 planes, viai_bf3.h) with the scales of *amax / *xmax
    ConvGeom g;                        // forward geometry (ly = lx = 1)
};

// Weight image of a launch (the values are those of viai_pack_job.frag: the packed formats themselves)
enum WLayout : int { WL_PLANAR_BF3 = 0, WL_FRAG_BF3 = 1, WL_F32 = 2, WL_FRAG_F16 = 3, WL_PLANAR_F16 = 4 };
static inline bool wl_f16(int l) { return l == WL_FRAG_F16 || l == WL_PLANAR_F16; }
static inline bool wl_frag(int l) { return l == WL_FRAG_BF3 || l == WL_FRAG_F16; }

// One value per launcher that is really distinct; tile instances within a family are the family's own business.
enum ConvKernel : int {
    CK_NONE = 0,            // the entry point refuses the call
    CK_DIRECT,              // Cin = 1 / Cout = 1 streaming kernels (conv_direct.hip)
    CK_STEM,                // 7 x 7 stride-2 image conv (conv_stem.hip)
    CK_IGEMM_F32, CK_IGEMM_BF3, CK_IGEMM_SK,
    CK_HALO, CK_HALO_C32, CK_HALO_C32_DMA,
    CK_HALO_WIDE, CK_WIDE_DMA_S1, CK_WIDE_DMA_S2, CK_LIN_DMA,
    CK_DGRAD_S2, CK_DGRAD_S2_PATCH,
    CK_WGRAD_MFMA, CK_WGRAD32, CK_WGRAD_BF3, CK_WGRAD_PATCH, CK_WGRAD_STEM
};

// Everything conv_api.hip decides about one launch, decided once (route_fwd / route_dgrad / route_wgrad).  The geometry goes into the
// argument block of the launch (ConvArgs::g / WgradArgs::g), built once by the same function.
struct ConvRoute {
    bool ok;                // the entry point accepts the call (a data gradient whose classes are all tapless is accepted and launches nothing)
    int kernel;             // ConvKernel
    int layout;             // WLayout of the weight image the kernel reads
    const char* family;     // what viai_conv2d_last_kernel reports after the launch
    int launches;           // conv-kernel launches of the call
    bool bf3;               // the layer runs on the split-precision (bf16x3 / f16x2) kernels in this direction
    bool f16;               // ... and has an f16x2 form there (the abs-max of the activation operand matters)
    // forward: BatchNorm partial geometry -- rows per partial block, or th x tw tiles clipped at the map's edge
    int stat_rows, tile_h, tile_w;
    // data gradient
    bool fused, zero_fill;  // all parity classes in one launch / a class without a tap gets zeros first
    bool halo;              // the classes run on the small-channel halo kernels
    // weight gradient
    int ksplit;
    // which operands of the direction may arrive pre-split (VIAI_P16_OK_* bits)
    int p16;
};

// 3 x 3 window of a tap table: origin (y0, x0) and, per window position row * 3 + col, the weight slot; false unless all nine positions
// are present exactly within the window
static inline bool viai_window9(const ConvGeom& g, int* y0, int* x0, int* slots9) {
    if (g.ntaps != 9) return false;
    int yy = g.dy[0], xx = g.dx[0];
    for (int t = 1; t < 9; ++t) { yy = g.dy[t] < yy ? g.dy[t] : yy; xx = g.dx[t] < xx ? g.dx[t] : xx; }
    unsigned seen = 0;
    for (int t = 0; t < 9; ++t) {
        const int r = g.dy[t] - yy, c = g.dx[t] - xx;
        if (r > 2 || c > 2) return false;
        seen |= 1u << (r * 3 + c);
        if (slots9) slots9[r * 3 + c] = g.ws[t];
    }
    if (y0) *y0 = yy;
    if (x0) *x0 = xx;
    return seen == 0x1ffu;
}

// conv_igemm.hip: exact-fp32 MFMA kernels
bool viai_conv_igemm_ok(int C1, int C2, int Cout, int OC1);
const char* viai_conv_igemm_family(long M, int n_out);
int viai_conv_igemm_launch(ConvArgs& a, hipStream_t st);
int viai_igemm_tile_m(long M, int n_out);
// conv_igemm_bf3.hip: bf16x3 / f16x2 implicit GEMM (tile instance by layout, rows and channels) and its 32 x 32 split-K kernel
const char* viai_conv_igemm_bf3_family(int layout, long M, int n_out);
int viai_conv_igemm_bf3_launch(ConvArgs& a, hipStream_t st);
int viai_conv_igemm_sk_launch(ConvArgs& a, hipStream_t st);
size_t viai_bf3_packed_floats(int n_out, int k_in, int taps);
int viai_pack_weight_bf3(const float* w, void* wp, int n_out, int k_in, int taps, long s_no, long s_ki, int frag, hipStream_t st);
int viai_pack_job_bf3(const float* w, void* wp, int n_out, int k_in, int taps, long s_no, long s_ki, int frag, viai_pack_job* job);
bool viai_bf3_frag_layout(long M, int n_out);
bool viai_bf3_sk_ok(long M, int n_out, int C1, int C2);
// conv_halo_bf3.hip: LDS-resident tiles, small-channel (halo, halo_c32 with the filter in registers) and wide
bool viai_conv_halo_ok(const ConvGeom& g, int C1, int C2, int Cout);
bool viai_conv_halo16_ok(const ConvGeom& g, int C1, int C2, int Cout);
int viai_conv_halo_bf3_launch(ConvArgs& a, hipStream_t st);
int viai_conv_halo_c32_launch(ConvArgs& a, hipStream_t st);
bool viai_conv_halo_wide_ok(const ConvArgs& a);
const char* viai_conv_halo_wide_family(const ConvArgs& a);
int viai_halo_tiles_y(const ConvGeom& g);      // 8 x 16 output tiles of the wide halo kernel (the last row / column of tiles may be partial)
int viai_halo_tiles_x(const ConvGeom& g);
int viai_halo_s2_rows(const ConvGeom& g);      // tile rows (8 or 4) of the stride-2 forward of the wide layers: BatchNorm partial blocks = 16 x rows pixels
int viai_conv_halo_wide_launch(ConvArgs& a, hipStream_t st);
// conv_halo_dma.hip: P16 input patches by LDS-DMA
bool viai_halo_dma_on();
bool viai_conv_halo_c32_dma_ok(const ConvArgs& a);
int viai_conv_halo_c32_dma_launch(ConvArgs& a, hipStream_t st);
bool viai_conv_s2_dma_ok(const ConvArgs& a);          // stride-2 forward, loader / consumer waves
int viai_conv_s2_dma_launch(ConvArgs& a, hipStream_t st);
bool viai_conv_s1_dma_ok(const ConvArgs& a);          // stride-1 256 k-channel layers on the same kernel (D.conv3)
int viai_conv_s1_dma_launch(ConvArgs& a, hipStream_t st);
bool viai_conv_lin_dma_geom_ok(const ConvArgs& a);   // stride-1 3 x 3 layers on linear pixel tiles (maps that are not whole 8 x 16 tiles: the ResNet branch)
int viai_conv_lin_dma_launch(ConvArgs& a, hipStream_t st);
int viai_lin_dma_stat_merge(long M, int Cout, int* grid, int* pw, int* nitems);   // > 0: the kernel's BatchNorm partials are merged per block (that many per channel)
// conv_stem.hip: the 7 x 7 stride-2 image conv of the ResNet branch on the f16x2 matrix-core path (forward + weight gradient)
bool viai_conv_stem_ok(const ConvGeom& g, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw);
int viai_conv_stem_fwd_launch(ConvArgs& a, hipStream_t st);
int viai_conv_stem_wgrad_slabs(const ConvGeom& g);
int viai_conv_stem_wgrad_launch(WgradArgs& a, int Cin, float* dw, int accumulate, hipStream_t st);
int viai_conv_stem_pack(const float* w, float* wp, int Cin, hipStream_t st);
// conv_dgrad_s2_bf3.hip: 3 x 3 stride-2 data gradient, the four parity classes in one launch (gather kernel, or patch-staged for f16x2)
bool viai_dgrad_s2_ok(const viai_conv2d* c);
bool viai_dgrad_s2_patch_ok(const viai_conv2d* c);
int viai_conv_dgrad_s2_bf3_launch(ConvArgs& a, hipStream_t st);
int viai_conv_dgrad_s2_patch_launch(ConvArgs& a, hipStream_t st);
// weight gradients: conv_wgrad.hip (fp32 MFMA, all-taps 32-channel), conv_wgrad_bf3.hip, conv_wgrad_patch.hip
bool viai_wgrad_mfma_ok(int Cout, int C1, int C2);
int viai_wgrad_mfma_launch(WgradArgs& a, int ksplit, hipStream_t st);
bool viai_wgrad32_ok(const ConvGeom& g, int Cout, int C1, int C2);
int viai_wgrad32_ksplit(long M);
int viai_wgrad32_launch(WgradArgs& a, int ksplit, hipStream_t st);
int viai_wgrad_bf3_launch(WgradArgs& a, int ksplit, hipStream_t st);
bool viai_wgrad_bf3_ok(int Cout, int C1, int C2);
int viai_wgrad_pick_ksplit(int Cout, int Cin, int ntaps, long M);
int viai_wgrad_patch_cfg(const ConvGeom& g, int Cout, int C1, int C2, bool switches);   // instance that takes the layer (0: none); switches: honour VIAI_WGRAD_PATCH_S2
const char* viai_wgrad_patch_family(int cfg);
int viai_wgrad_patch_ksplit(const ConvGeom& g, int Cout, int C1, int C2);
int viai_wgrad_patch_launch(WgradArgs& a, hipStream_t st);

// Which kernel family ran: conv_api.hip tags every launch with its route's family; the C-ABI entry points reset the tag on entry and
// viai_conv2d_last_kernel() reports it (bench.py prices each family against the ceiling of its arithmetic -- the name ends in
// _f16x2 / _bf16x3 / _f32, or is "direct" for the Cin = 1 / Cout = 1 streaming kernels).  Per thread, like the error slot.
struct ViaiKernelTag { const char* family; int launches; };
extern thread_local ViaiKernelTag viai_kernel_tag;
static inline void viai_tag_kernel(const char* family) { viai_kernel_tag.family = family; viai_kernel_tag.launches += 1; }
static inline void viai_tag_reset() { viai_kernel_tag.family = nullptr; viai_kernel_tag.launches = 0; }

// geometry builders (conv_api.hip)
void viai_geom_fwd(const viai_conv2d* c, ConvGeom* g);
int viai_geom_dgrad_class(const viai_conv2d* c, int a, int b, ConvGeom* g);   // returns ntaps
