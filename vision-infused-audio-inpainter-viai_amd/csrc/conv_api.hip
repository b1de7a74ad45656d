// C-ABI entry points of the convolution family: geometry (tap tables), weight
// packing, and dispatch between the MFMA implicit-GEMM kernels and the
// streaming kernels for the Cin == 1 / Cout == 1 layers.
#include "viai_common.h"
#include "viai_internal.h"
#include <cstdlib>
#include <cstring>

// direct kernels (conv_direct.hip)
int viai_cin1_fwd(const viai_conv2d* c, const float* x, const float* w, const float* bias, float* y, float* stat, int act, hipStream_t st);
int viai_cin1_stat_geom(const viai_conv2d* c, int* nblk, int* rows);
int viai_cin1_dgrad(const viai_conv2d* c, const float* dy, const float* w, float* dx, hipStream_t st);
size_t viai_cin1_wgrad_ws_floats(const viai_conv2d* c);
int viai_cin1_wgrad(const viai_conv2d* c, const float* x, const float* dy, float* ws, float* dw, int accumulate, hipStream_t st);
int viai_cout1_fwd(const viai_conv2d* c, const float* x, const float* wp, const float* bias, float* y, int act, hipStream_t st);
int viai_cout1_dgrad(const viai_conv2d* c, const float* dy, const float* wp, float* dx, hipStream_t st);
size_t viai_cout1_wgrad_ws_floats(const viai_conv2d* c);
int viai_cout1_wgrad(const viai_conv2d* c, const float* x, const float* dy, float* ws, float* dw, int accumulate, hipStream_t st);
int viai_wgrad_reduce(const float* ws, float* dw, int nz, int T, int Cout, int Cin, long s_co, long s_ci, int accumulate, hipStream_t st);
extern "C" int viai_colsum_blocks(long M, int C);
extern "C" int viai_colsum(const float* x, long M, int C, float* part, float* out, int accumulate, void* stream);

static inline int cin_of(const viai_conv2d* c) { return c->C1 + c->C2; }
static inline int dil_h(const viai_conv2d* c) { return c->dh > 1 ? c->dh : 1; }
static inline int dil_w(const viai_conv2d* c) { return c->dw > 1 ? c->dw : 1; }
static inline int pad_b(const viai_conv2d* c) { return c->ph2 >= 0 ? c->ph2 : c->ph; }
static inline int pad_r(const viai_conv2d* c) { return c->pw2 >= 0 ? c->pw2 : c->pw; }
enum { K_IGEMM = 0, K_CIN1 = 1, K_COUT1 = 2, K_RUN = 3 };
static inline int kind_of(const viai_conv2d* c) {
    if (cin_of(c) == 1) return K_CIN1;
    if (c->Cout == 1) return K_COUT1;
    if (cin_of(c) <= 4) return K_RUN;       // ResNet conv1 (Cin 3 / 2): input stored with channel stride 4
    return K_IGEMM;
}

// the Cin = 1 streaming kernels exist for these windows and channel counts only (conv_direct.hip)
static inline bool cin1_ok(const viai_conv2d* c) {
    const bool win = (c->kh == 3 && c->kw == 3) || (c->kh == 1 && (c->kw == 1 || c->kw == 3 || c->kw == 4 || c->kw == 6));
    return win && (c->Cout == 32 || c->Cout == 64 || c->Cout == 128);
}
static inline bool valid(const viai_conv2d* c) {
    if (!c || c->N <= 0 || c->IH <= 0 || c->IW <= 0 || c->C1 <= 0 || c->C2 < 0 || c->Cout <= 0) return false;
    if (cin_of(c) == 1 && !cin1_ok(c)) return false;
    const bool runk = (cin_of(c) > 1 && cin_of(c) <= 4 && c->Cout > 1);     // row-run kind: taps are kernel rows
    if (c->kh <= 0 || c->kw <= 0) return false;
    if (runk ? (c->kh > VIAI_MAX_TAPS || c->kw > 8) : (c->kh * c->kw > VIAI_MAX_TAPS)) return false;
    if (c->sh <= 0 || c->sw <= 0 || c->ph < 0 || c->pw < 0) return false;
    if (c->transposed && (c->sh != 1 || c->sw != 1)) return false;
    if ((dil_h(c) > 1 || dil_w(c) > 1 || c->ph2 >= 0 || c->pw2 >= 0) && (c->transposed || kind_of(c) != K_IGEMM)) return false;
    if (cin_of(c) > 1 && cin_of(c) <= 4 && c->Cout > 1 && (c->kw > 8 || c->transposed || c->C2 != 0)) return false;
    int oh, ow;
    viai_conv2d_out_hw(c, &oh, &ow);
    return oh > 0 && ow > 0;
}
// ---- math mode of the contraction-shaped layers ------------------------------------------------------
// default: "bf16x3" split-bf16 MFMA (fp32-grade accuracy, 2.67x the fp32-MFMA ceiling) wherever the
// 128x128 tile applies; VIAI_MATH=fp32 forces the exact-fp32 MFMA kernels everywhere.
static bool bf3_enabled() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("VIAI_MATH"); v = (e && (!strcmp(e, "fp32") || !strcmp(e, "f32"))) ? 0 : 1; }
    return v == 1;
}
// f16x2 (two fp16 terms per operand) for every split-precision kernel that has the form; VIAI_F16X2=0 keeps them on bf16x3
static bool f16x2_enabled() {
    static int on = -1;
    if (on < 0) { const char* e = getenv("VIAI_F16X2"); on = e ? atoi(e) : 1; }
    return on != 0;
}

extern "C" int viai_abi_version(void) { return VIAI_ABI_VERSION; }

thread_local ViaiKernelTag viai_kernel_tag = {nullptr, 0};
// name of the kernel family the LAST convolution entry point of this thread (viai_conv2d_fwd / _dgrad[_f16] / _wgrad[_f16] /
// viai_conv2d_cin1_bn_*) launched, copied into buf (NUL-terminated, truncated to cap); returns the number of conv-kernel launches of
// that call (a strided data gradient on the gather kernel is one launch per parity class), 0 if none.
static void copy_name(char* buf, int cap, const char* s) {
    if (buf != nullptr && cap > 0) { strncpy(buf, s ? s : "", cap - 1); buf[cap - 1] = 0; }
}
extern "C" int viai_conv2d_last_kernel(char* buf, int cap) {
    copy_name(buf, cap, viai_kernel_tag.family);
    return viai_kernel_tag.launches;
}

extern "C" int viai_conv2d_out_hw(const viai_conv2d* c, int* OH, int* OW) {
    if (c->transposed) {   // ConvTranspose2d, stride 1: (I-1) - 2p + k
        *OH = c->IH - 1 - 2 * c->ph + c->kh;
        *OW = c->IW - 1 - 2 * c->pw + c->kw;
    } else {
        *OH = (c->IH + c->ph + pad_b(c) - dil_h(c) * (c->kh - 1) - 1) / c->sh + 1;
        *OW = (c->IW + c->pw + pad_r(c) - dil_w(c) * (c->kw - 1) - 1) / c->sw + 1;
    }
    return 0;
}

extern "C" size_t viai_conv2d_packed_floats(const viai_conv2d* c) {
    if (kind_of(c) == K_RUN) return (size_t)c->Cout * c->kh * 32;
    size_t n = (size_t)c->Cout * cin_of(c) * c->kh * c->kw;
    if (kind_of(c) == K_IGEMM && bf3_enabled()) {                                  // room for fragment-major bf16 planes (fwd or dgrad form)
        size_t f = viai_bf3_packed_floats(c->Cout, cin_of(c), c->kh * c->kw), d = viai_bf3_packed_floats(cin_of(c), c->Cout, c->kh * c->kw);
        size_t m = f > d ? f : d;
        return m > n ? m : n;
    }
    return n;
}

static void geom_base(const viai_conv2d* c, ConvGeom* g) {
    int oh, ow;
    viai_conv2d_out_hw(c, &oh, &ow);
    g->run = 0;
    g->N = c->N; g->IH = c->IH; g->IW = c->IW; g->OH = oh; g->OW = ow; g->SH = oh; g->SW = ow;
    g->ly = g->lx = 1; g->ay = g->ax = 0;
    g->my = c->sh; g->mx = c->sw;
}

void viai_geom_fwd(const viai_conv2d* c, ConvGeom* g) {
    geom_base(c, g);
    g->ntaps = g->wtaps = c->kh * c->kw;
    for (int r = 0; r < c->kh; ++r)
        for (int s = 0; s < c->kw; ++s) {
            int t = r * c->kw + s;
            g->dy[t] = (c->transposed ? c->ph - r : r * dil_h(c) - c->ph);
            g->dx[t] = (c->transposed ? c->pw - s : s * dil_w(c) - c->pw);
            g->ws[t] = t;
        }
}

// row-run geometry (1 < Cin <= 4): one "tap" per kernel row, K = 8 pixels x 4 channels per tap
static void geom_run(const viai_conv2d* c, ConvGeom* g) {
    geom_base(c, g);
    g->run = 1;
    g->ntaps = g->wtaps = c->kh;
    for (int r = 0; r < c->kh; ++r) { g->dy[r] = r - c->ph; g->dx[r] = -c->pw; g->ws[r] = r; }
}

// wp[co][r][s*4+ch] = w[co][ch][r][s], zero for s >= kw or ch >= Cin
__global__ void pack_run_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int kh, int kw) {
    const int total = Cout * kh * 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int k = i % 32, r = (i / 32) % kh, co = i / (32 * kh);
        int s_ = k / 4, ch = k % 4;
        wp[i] = (s_ < kw && ch < Cin) ? w[((size_t)(co * Cin + ch) * kh + r) * kw + s_] : 0.f;
    }
}

// dw[co][ch][r][s] (+)= sum_z ws[z][r][co][s*4+ch]
__global__ void wgrad_reduce_run_kernel(const float* __restrict__ ws, float* __restrict__ dw, int nz, int Cout, int Cin,
                                        int kh, int kw, int accumulate) {
    const int total = Cout * Cin * kh * kw;
    const size_t slab = (size_t)kh * Cout * 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int s_ = i % kw, r = (i / kw) % kh, ch = (i / (kw * kh)) % Cin, co = i / (kw * kh * Cin);
        size_t src = ((size_t)r * Cout + co) * 32 + s_ * 4 + ch;
        float acc = 0.f;
        for (int z = 0; z < nz; ++z) acc += ws[z * slab + src];
        dw[i] = accumulate ? dw[i] + acc : acc;
    }
}

// data gradient: produced tensor = dx (N, IH, IW, Cin), gathered tensor = dy (N, OH, OW, Cout).
// class (a, b) = (iy mod sh, ix mod sw).
int viai_geom_dgrad_class(const viai_conv2d* c, int a, int b, ConvGeom* g) {
    int oh, ow;
    viai_conv2d_out_hw(c, &oh, &ow);
    g->N = c->N; g->IH = oh; g->IW = ow;           // gathered = dy
    g->OH = c->IH; g->OW = c->IW;                  // produced = dx
    g->ly = c->sh; g->lx = c->sw; g->ay = a; g->ax = b;
    g->SH = (c->IH - a + c->sh - 1) / c->sh;
    g->SW = (c->IW - b + c->sw - 1) / c->sw;
    g->my = g->mx = 1;
    g->run = 0;
    g->wtaps = c->kh * c->kw;
    int nt = 0;
    for (int r = 0; r < c->kh; ++r)
        for (int s = 0; s < c->kw; ++s) {
            int dy, dx;
            if (c->transposed) {                   // fwd: o = i - p + r  ->  gathered y = iy + (r - p)
                dy = r - c->ph; dx = s - c->pw;
            } else {                               // fwd: i = o*s - p + r ->  o = (iy + p - r)/s
                int ny = a + c->ph - r * dil_h(c), nx = b + c->pw - s * dil_w(c);
                if (((ny % c->sh) + c->sh) % c->sh != 0 || ((nx % c->sw) + c->sw) % c->sw != 0) continue;
                dy = ny / c->sh; dx = nx / c->sw;   // exact (divisible), may be negative
            }
            g->dy[nt] = dy; g->dx[nt] = dx; g->ws[nt] = r * c->kw + s;
            ++nt;
        }
    g->ntaps = nt;
    return nt;
}

// ---- routes ----------------------------------------------------------------------------------------------
// One function per direction decides everything about a launch -- kernel, weight image, BatchNorm partial geometry, P16 mask -- from the
// descriptor and the operand form.  The geometry is built once, into the argument block the launch will use; the family predicates (in the
// files that own their tile constants) are each asked once.  The entry points, the pack functions and every query below read the route.
//
// The layer-level fields (layout of the fp32 / abs-max forms, stat_rows / tile_h / tile_w, p16, bf3, ksplit) do not depend on the form: the
// fp32 and P16 forwards of one layer share one `stat` buffer and one weight image.  The one exception is `lin`: a P16 forward on the
// linear-tile kernel writes its partials per 128 consecutive pixels, so layers reporting VIAI_P16_OK_FWD_LIN finalize with viai_bn_finalize_lin.

static bool stem_layer(const viai_conv2d* c, const ConvGeom& g) {
    return f16x2_enabled() && bf3_enabled() && !c->transposed && viai_conv_stem_ok(g, cin_of(c), c->Cout, c->kh, c->kw, c->sh, c->sw, c->ph, c->pw);
}

// the split-precision kernel of one launch (forward, or one parity class of a data gradient, as a.g says), in the order they are preferred
static void pick_split_kernel(ConvRoute& r, const ConvArgs& a, bool halo, bool wide, bool lin, bool p16) {
    const bool oc_ok = a.OC1 % 32 == 0 || a.OC1 == a.Cout;
    if (halo) {
        if (!oc_ok) return;
        if (r.layout == WL_FRAG_F16 && viai_conv_halo16_ok(a.g, a.C1, a.C2, a.Cout)) {
            r.kernel = (p16 && viai_conv_halo_c32_dma_ok(a)) ? CK_HALO_C32_DMA : CK_HALO_C32; r.family = "halo_c32_f16x2";
        } else { r.kernel = CK_HALO; r.family = r.layout == WL_FRAG_F16 ? "halo_f16x2" : "halo_bf16x3"; }
        return;
    }
    if (!oc_ok || (a.C2 > 0 && a.C1 % 32 != 0)) return;
    if (!wl_frag(r.layout) && viai_bf3_sk_ok(a.M, a.Cout, a.C1, a.C2)) {
        r.kernel = CK_IGEMM_SK; r.family = r.layout == WL_PLANAR_F16 ? "igemm_sk32x32_f16x2" : "igemm_sk32x32_bf16x3";
    } else if (p16 && lin) { r.kernel = CK_LIN_DMA; r.family = "lin_dma_f16x2"; }
    else if (wide) {
        if (p16 && a.g.my == 2 && viai_conv_s2_dma_ok(a)) { r.kernel = CK_WIDE_DMA_S2; r.family = "halo_wide_s2_f16x2"; }
        else if (p16 && a.g.my == 1 && viai_conv_s1_dma_ok(a)) { r.kernel = CK_WIDE_DMA_S1; r.family = "halo_wide256_f16x2"; }
        else { r.kernel = CK_HALO_WIDE; r.family = viai_conv_halo_wide_family(a); }
    } else if (!p16) { r.kernel = CK_IGEMM_BF3; r.family = viai_conv_igemm_bf3_family(r.layout, a.M, a.Cout); }      // only the patch-staged kernels stage P16 pieces
}
// the family tag comes from the route: the launchers launch what they are told and name nothing
static int launch_conv_kernel(const ConvRoute& r, ConvArgs& a, hipStream_t st) {
    if (r.kernel == CK_NONE) return (int)hipErrorInvalidValue;
    viai_tag_kernel(r.family);
    switch (r.kernel) {
    case CK_STEM: return viai_conv_stem_fwd_launch(a, st);
    case CK_IGEMM_F32: return viai_conv_igemm_launch(a, st);
    case CK_DGRAD_S2: return viai_conv_dgrad_s2_bf3_launch(a, st);
    case CK_DGRAD_S2_PATCH: return viai_conv_dgrad_s2_patch_launch(a, st);
    case CK_HALO: return viai_conv_halo_bf3_launch(a, st);
    case CK_HALO_C32: return viai_conv_halo_c32_launch(a, st);
    case CK_HALO_C32_DMA: return viai_conv_halo_c32_dma_launch(a, st);
    case CK_IGEMM_SK: return viai_conv_igemm_sk_launch(a, st);
    case CK_IGEMM_BF3: return viai_conv_igemm_bf3_launch(a, st);
    case CK_LIN_DMA: return viai_conv_lin_dma_launch(a, st);
    case CK_HALO_WIDE: return viai_conv_halo_wide_launch(a, st);
    case CK_WIDE_DMA_S1: return viai_conv_s1_dma_launch(a, st);
    case CK_WIDE_DMA_S2: return viai_conv_s2_dma_launch(a, st);
    default: return (int)hipErrorInvalidValue;
    }
}
static void pick_f32_kernel(ConvRoute& r, const ConvArgs& a) {
    if (!viai_conv_igemm_ok(a.C1, a.C2, a.Cout, a.OC1)) return;
    r.kernel = CK_IGEMM_F32; r.family = viai_conv_igemm_family(a.M, a.Cout);
}

// forward.  Order: direct (Cin = 1 / Cout = 1), stem, fp32 igemm (VIAI_MATH=fp32 or Cin not in sixteens), then pick_split_kernel
static ConvRoute route_fwd(const viai_conv2d* c, int form, ConvArgs& a) {
    ConvRoute r{};
    const int kind = kind_of(c);
    const bool p16 = (form & 3) == VIAI_FORM_P16, f16 = f16x2_enabled();
    r.layout = WL_F32; r.launches = 1; r.stat_rows = 128;
    a.C1 = c->C1; a.C2 = c->C2; a.Cout = c->Cout; a.OC1 = c->Cout; a.in_p16 = p16;
    if (kind == K_CIN1 || kind == K_COUT1) {
        if (!p16) { r.kernel = CK_DIRECT; r.family = "direct"; }
        return r;
    }
    if (kind == K_RUN) { geom_run(c, &a.g); a.C1 = 32; a.C2 = 0; }
    else viai_geom_fwd(c, &a.g);
    const ConvGeom& g = a.g;
    a.M = g.N * g.OH * g.OW;
    const long M = (long)g.N * g.OH * g.OW;
    r.bf3 = kind == K_IGEMM && bf3_enabled() && cin_of(c) % 16 == 0;
    if (!r.bf3) {
        const bool stem = kind == K_RUN && stem_layer(c, g);
        if (!stem) r.stat_rows = viai_igemm_tile_m(M, c->Cout);
        r.f16 = stem;
        if (stem && !p16) { r.kernel = CK_STEM; r.family = "stem_f16x2"; }
        else if (!p16) pick_f32_kernel(r, a);
        return r;
    }
    const bool halo = viai_conv_halo_ok(g, c->C1, c->C2, c->Cout);
    const bool wide = f16 && viai_conv_halo_wide_ok(a), lin = f16 && viai_conv_lin_dma_geom_ok(a);
    // weight image: fragment-major for the wide-tile, halo and linear-tile kernels, planar (staged in LDS) otherwise
    r.layout = (halo || viai_bf3_frag_layout(M, c->Cout)) ? (f16 ? WL_FRAG_F16 : WL_FRAG_BF3) : (wide || lin) ? WL_FRAG_F16 : f16 ? WL_PLANAR_F16 : WL_PLANAR_BF3;
    a.wfrag = r.layout;
    if (!halo && !wide) r.stat_rows = (!wl_frag(r.layout) && viai_bf3_sk_ok(M, c->Cout, c->C1, c->C2)) ? 32 : viai_igemm_tile_m(M, c->Cout);
    if (!halo && wide && c->sh == 2) r.stat_rows = 16 * viai_halo_s2_rows(g);          // stride-2 wide forward: 64-pixel tiles where it runs them
    if (wide && (g.OH % 8 != 0 || g.OW % 16 != 0)) { r.tile_h = 8; r.tile_w = 16; }    // the wide halo kernel's 8 x 16 tiles, clipped at the map's edge
    if (f16 && c->C2 == 0 && (halo || wide || lin)) r.p16 = VIAI_P16_OK_FWD_X | (lin ? VIAI_P16_OK_FWD_LIN : 0);
    r.f16 = wl_f16(r.layout);
    if (!p16 || r.p16) pick_split_kernel(r, a, halo, wide, lin, p16);
    return r;
}

// data gradient (a: parity class (0, 0)).  Order: direct, fp32 igemm class by class, the fused stride-2 kernels, then pick_split_kernel class by class
static ConvRoute route_dgrad(const viai_conv2d* c, int form, ConvArgs& a) {
    ConvRoute r{};
    const int kind = kind_of(c), Cin = cin_of(c);
    const bool p16 = (form & 3) == VIAI_FORM_P16, amax = (form & 3) != VIAI_FORM_F32, f16 = f16x2_enabled();
    r.layout = WL_F32;
    if (kind == K_RUN) return r;                            // image inputs need no data gradient
    if (kind != K_IGEMM) {
        if (!amax) { r.kernel = CK_DIRECT; r.family = "direct"; r.launches = 1; r.ok = true; }
        return r;
    }
    a.C1 = c->Cout; a.C2 = 0; a.Cout = Cin; a.OC1 = c->C1;        // produced tensor = dx, gathered tensor = dy: the channel roles swapped
    a.in_p16 = p16;
    const bool unit = c->sh == 1 && c->sw == 1;
    bool halo = c->sw == 1 && (c->sh == 1 || (c->sh == 2 && f16 && !c->transposed));       // (the stride-(2, 1) layer: both row-parity classes on the halo kernel)
    ConvArgs last = a;                                      // the last class that launches names the family
    for (int a_ = 0; a_ < c->sh; ++a_)
        for (int b_ = 0; b_ < c->sw; ++b_) {
            ConvGeom tmp;
            ConvGeom& g = (a_ == 0 && b_ == 0) ? a.g : tmp;
            const int nt = viai_geom_dgrad_class(c, a_, b_, &g);
            if (g.SH <= 0 || g.SW <= 0) continue;
            if (nt == 0) { r.zero_fill = true; halo = false; continue; }         // a class with no valid tap (e.g. 1x1 stride 2) receives no gradient
            halo = halo && viai_conv_halo_ok(g, c->Cout, 0, Cin);
            r.launches += 1;
            last.g = g;
        }
    last.M = last.g.N * last.g.SH * last.g.SW;
    a.M = a.g.N * a.g.SH * a.g.SW;
    r.bf3 = r.launches == 0 || (bf3_enabled() && c->Cout % 16 == 0);
    r.f16 = f16 && r.bf3;
    if (amax && !r.f16) return r;
    if (!r.bf3) {
        pick_f32_kernel(r, last);
        r.ok = r.kernel != CK_NONE;
        return r;
    }
    halo = halo && r.launches > 0;
    const bool s2 = viai_dgrad_s2_ok(c);
    const bool live0 = unit && r.launches == 1;
    const bool wide = f16 && live0 && viai_conv_halo_wide_ok(a), lin = f16 && live0 && viai_conv_lin_dma_geom_ok(a);
    const bool frag = halo || s2 || viai_bf3_frag_layout((long)c->N * ((c->IH + c->sh - 1) / c->sh) * ((c->IW + c->sw - 1) / c->sw), Cin);
    r.layout = amax ? ((frag || wide || lin) ? WL_FRAG_F16 : WL_PLANAR_F16) : frag ? WL_FRAG_BF3 : WL_PLANAR_BF3;
    a.wfrag = last.wfrag = r.layout;
    if (f16 && (s2 || (unit && (halo || wide || lin)))) r.p16 = VIAI_P16_OK_DGRAD_DY;
    if (p16 && !r.p16) return r;
    if (s2) {                                               // all four parity classes in one launch
        r.fused = r.ok = true; r.launches = 1;
        if (amax && viai_dgrad_s2_patch_ok(c)) { r.kernel = CK_DGRAD_S2_PATCH; r.family = "dgrad_s2_patch_f16x2"; }
        else { r.kernel = CK_DGRAD_S2; r.family = amax ? "dgrad_s2_f16x2" : "dgrad_s2_bf16x3"; }
        return r;
    }
    r.halo = halo;
    if (r.launches > 0) pick_split_kernel(r, last, halo, amax && wide, amax && lin, p16);       // (the patch-staged kernels are f16x2 only)
    r.ok = r.launches == 0 || r.kernel != CK_NONE;
    return r;
}

// weight gradient.  Order: direct, stem (f16x2 forms), patch (f16x2 forms), all-taps 32, bf3, fp32 MFMA
static ConvRoute route_wgrad(const viai_conv2d* c, int form, WgradArgs& a) {
    ConvRoute r{};
    const int kind = kind_of(c), flags = (form & 3) == VIAI_FORM_P16 ? (form >> 2) : 0;
    const bool amax = (form & 3) != VIAI_FORM_F32;
    r.layout = WL_F32; r.ksplit = 1;
    int oh, ow; viai_conv2d_out_hw(c, &oh, &ow);
    const long M = (long)c->N * oh * ow;
    a.C1 = c->C1; a.C2 = c->C2; a.Cout = c->Cout; a.M = (int)M;
    a.dy_p16 = (flags & VIAI_P16_DY) ? 1 : 0; a.x_p16 = (flags & VIAI_P16_X) ? 1 : 0;
    if (kind == K_CIN1 || kind == K_COUT1) {
        if (!amax) { r.kernel = CK_DIRECT; r.family = "direct"; r.launches = 1; r.ok = true; }
        return r;
    }
    if (kind == K_RUN) {
        a.C1 = 32; a.C2 = 0;
        geom_run(c, &a.g);
        r.f16 = stem_layer(c, a.g);
        if (amax && r.f16 && !flags) { r.kernel = CK_WGRAD_STEM; r.family = "wgrad_stem_f16x2"; r.ksplit = viai_conv_stem_wgrad_slabs(a.g); }
        else if (!amax) {
            r.ksplit = viai_wgrad_pick_ksplit(c->Cout, 32, c->kh, M);
            if (viai_wgrad_mfma_ok(c->Cout, 32, 0)) { r.kernel = CK_WGRAD_MFMA; r.family = "wgrad_mfma_f32"; }
        }
        r.launches = r.ok = r.kernel != CK_NONE;
        return r;
    }
    viai_geom_fwd(c, &a.g);
    const bool split = f16x2_enabled() && bf3_enabled(), w32 = viai_wgrad32_ok(a.g, c->Cout, c->C1, c->C2), wbf3 = viai_wgrad_bf3_ok(c->Cout, c->C1, c->C2);
    const int cfg = split ? viai_wgrad_patch_cfg(a.g, c->Cout, c->C1, c->C2, true) : 0;
    r.ksplit = w32 ? viai_wgrad32_ksplit(M) : viai_wgrad_pick_ksplit(c->Cout, cin_of(c), c->kh * c->kw, M);
    r.f16 = split && (wbf3 || cfg != 0);
    if (cfg != 0) r.p16 = VIAI_P16_OK_WGRAD_DY | (c->C2 == 0 ? VIAI_P16_OK_WGRAD_X : 0);
    if ((amax && !r.f16) || (flags && cfg == 0) || ((flags & VIAI_P16_X) && c->C2 > 0)) return r;
    if (amax && cfg != 0) { r.kernel = CK_WGRAD_PATCH; r.family = viai_wgrad_patch_family(cfg); r.ksplit = viai_wgrad_patch_ksplit(a.g, c->Cout, c->C1, c->C2); }
    else if (w32) { r.kernel = CK_WGRAD32; r.family = "wgrad32_all_taps_f32"; }
    else if (bf3_enabled() && wbf3) { r.kernel = CK_WGRAD_BF3; r.family = amax ? "wgrad_bf3_f16x2" : "wgrad_bf3_bf16x3"; }
    else if (viai_wgrad_mfma_ok(c->Cout, c->C1, c->C2)) { r.kernel = CK_WGRAD_MFMA; r.family = "wgrad_mfma_f32"; }
    r.launches = r.ok = r.kernel != CK_NONE;
    return r;
}

extern "C" int viai_conv2d_route(const viai_conv2d* c, int pass, int form, char* family, int cap) {
    ConvRoute r{};
    if (valid(c) && form >= 0 && pass >= 0 && pass <= 2) {
        ConvArgs a{}; WgradArgs w{};
        r = pass == 0 ? route_fwd(c, form, a) : pass == 1 ? route_dgrad(c, form, a) : route_wgrad(c, form, w);
    }
    copy_name(family, cap, r.kernel != CK_NONE ? r.family : "");
    return r.kernel != CK_NONE ? r.launches : 0;
}

// ---- weight images -----------------------------------------------------------------------------------------
// One image: forward form [Cout][T][Cin] (dgrad = false) or data-gradient form [Cin][T][Cout], in the layout of the route that reads it;
// as a job of the batched pack when `job` is given, else packed now.  The streaming kernels share one fp32 image in both directions.
static int pack_image(const viai_conv2d* c, bool dgrad, int layout, const float* w, float* wp, viai_pack_job* job, void* stream) {
    const int T = c->kh * c->kw, Cin = cin_of(c), kind = kind_of(c);
    if (kind != K_IGEMM) { dgrad = false; layout = WL_F32; }
    const int n_out = dgrad ? Cin : c->Cout, k_in = dgrad ? c->Cout : Cin;
    const long s_co = c->transposed ? T : (long)Cin * T, s_ci = c->transposed ? (long)c->Cout * T : T;      // torch strides of the output / input channel
    const long s_no = kind == K_COUT1 ? 0 : dgrad ? s_ci : s_co, s_ki = dgrad ? s_co : s_ci;
    if (job != nullptr) return viai_pack_job_bf3(w, wp, n_out, k_in, T, s_no, s_ki, layout, job);
    if (layout == WL_F32) return viai_pack_weight(w, wp, n_out, k_in, T, s_no, s_ki, stream);
    return viai_pack_weight_bf3(w, wp, n_out, k_in, T, s_no, s_ki, layout, (hipStream_t)stream);
}

extern "C" int viai_conv2d_pack_fwd(const viai_conv2d* c, const float* w, float* wp, void* stream) {
    if (!valid(c)) return (int)hipErrorInvalidValue;
    ConvArgs a{};
    const ConvRoute r = route_fwd(c, VIAI_FORM_F32, a);
    if (kind_of(c) == K_RUN) {
        if (r.kernel == CK_STEM) return viai_conv_stem_pack(w, wp, cin_of(c), (hipStream_t)stream);
        int total = c->Cout * c->kh * 32;
        VIAI_LAUNCH(pack_run_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, wp, c->Cout, cin_of(c), c->kh, c->kw);
        return viai_launch_status();
    }
    return pack_image(c, false, r.layout, w, wp, nullptr, stream);
}

extern "C" int viai_conv2d_pack_dgrad(const viai_conv2d* c, const float* w, float* wp, void* stream) {
    if (!valid(c) || kind_of(c) == K_RUN) return (int)hipErrorInvalidValue;          // image inputs need no data gradient
    ConvArgs a{};
    return pack_image(c, true, route_dgrad(c, VIAI_FORM_F32, a).layout, w, wp, nullptr, stream);
}

// f16x2 data gradient: 1 if this layer has one (then pack with viai_conv2d_pack_dgrad_f16 and pass the abs-max of dy)
extern "C" int viai_conv2d_dgrad_f16_ok(const viai_conv2d* c) {
    if (!valid(c) || kind_of(c) != K_IGEMM) return 0;
    ConvArgs a{};
    return route_dgrad(c, VIAI_FORM_F32, a).f16 ? 1 : 0;
}

extern "C" int viai_conv2d_pack_dgrad_f16(const viai_conv2d* c, const float* w, float* wp, void* stream) {
    if (!viai_conv2d_dgrad_f16_ok(c)) return (int)hipErrorInvalidValue;
    ConvArgs a{};
    return pack_image(c, true, route_dgrad(c, VIAI_FORM_AMAX, a).layout, w, wp, nullptr, stream);
}

// Job descriptor of this layer's weight image for viai_pack_jobs_run (dgrad: 0 forward image, 1 data-gradient image, 2 its f16x2 form);
// returns 1 for the one image kind that is not batched (row-run mode of the image-input 7x7 conv: pack it with viai_conv2d_pack_fwd).
extern "C" int viai_conv2d_pack_job(const viai_conv2d* c, int dgrad, const float* w, float* wp, viai_pack_job* job) {
    if (!valid(c) || job == nullptr) return (int)hipErrorInvalidValue;
    if (kind_of(c) == K_RUN) return 1;
    ConvArgs a{};
    if (!dgrad || kind_of(c) != K_IGEMM) return pack_image(c, false, route_fwd(c, VIAI_FORM_F32, a).layout, w, wp, job, nullptr);
    if (dgrad == 2 && !viai_conv2d_dgrad_f16_ok(c)) return (int)hipErrorInvalidValue;
    return pack_image(c, true, route_dgrad(c, dgrad == 2 ? VIAI_FORM_AMAX : VIAI_FORM_F32, a).layout, w, wp, job, nullptr);
}

// ---- forward -------------------------------------------------------------------------------------------------
extern "C" int viai_conv2d_stat_geom(const viai_conv2d* c, int* nblk, int* rows_per_blk) {
    if (!valid(c)) return (int)hipErrorInvalidValue;
    if (kind_of(c) == K_CIN1) return viai_cin1_stat_geom(c, nblk, rows_per_blk);
    ConvArgs a{};
    const ConvRoute r = route_fwd(c, VIAI_FORM_F32, a);
    int oh, ow;
    viai_conv2d_out_hw(c, &oh, &ow);
    const long M = (long)c->N * oh * ow;
    *rows_per_blk = r.stat_rows;
    *nblk = r.tile_h > 0 ? c->N * ((oh + r.tile_h - 1) / r.tile_h) * ((ow + r.tile_w - 1) / r.tile_w) : (int)((M + r.stat_rows - 1) / r.stat_rows);
    return 0;
}

extern "C" int viai_conv2d_stat_tiles(const viai_conv2d* c, int* tile_h, int* tile_w) {
    if (!valid(c)) return (int)hipErrorInvalidValue;
    ConvArgs a{};
    const ConvRoute r = route_fwd(c, VIAI_FORM_F32, a);
    *tile_h = r.tile_h; *tile_w = r.tile_w;
    return 0;
}

// 1 if the forward launch of this layer splits its activations into fp16 terms (then x_amax matters)
extern "C" int viai_conv2d_fwd_f16_ok(const viai_conv2d* c) {
    if (!valid(c)) return 0;
    ConvArgs a{};
    const ConvRoute r = route_fwd(c, VIAI_FORM_F32, a);
    return r.f16 ? 1 : 0;
}

// x_amax: device float >= max |x| (and |x2|), or NULL.  The f16x2 kernels scale their activation operand by a power of two before the
// split: from x_amax when it is given (any magnitude is then representable), by the static 16 otherwise (|x| beyond 4094 saturates)
static int fwd_impl(const viai_conv2d* c, const float* x, const float* x2, const float* wp,
                    const float* bias, float* y, float* stat_part, int act, const float* x_amax, void* stream, int form) {
    if (!valid(c) || (c->C2 > 0) != (x2 != nullptr)) return (int)hipErrorInvalidValue;
    if (stat_part != nullptr && act != VIAI_ACT_NONE) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    viai_tag_reset();
    ConvArgs a{};
    const ConvRoute r = route_fwd(c, form, a);
    a.in = x; a.in2 = x2; a.wp = wp; a.bias = bias; a.out = y; a.out2 = nullptr; a.stat = stat_part;
    a.act = act; a.slope = 0.2f;
    if (r.f16) a.amax = x_amax;                              // f16x2 weight image = f16x2 kernel
    if (r.kernel != CK_DIRECT) return launch_conv_kernel(r, a, st);
    if (kind_of(c) == K_COUT1 && stat_part) return (int)hipErrorInvalidValue;
    viai_tag_kernel(r.family);
    return kind_of(c) == K_CIN1 ? viai_cin1_fwd(c, x, wp, bias, y, stat_part, act, st) : viai_cout1_fwd(c, x, wp, bias, y, act, st);
}
extern "C" int viai_conv2d_fwd(const viai_conv2d* c, const float* x, const float* x2, const float* wp,
                               const float* bias, float* y, float* stat_part, int act, void* stream) {
    return fwd_impl(c, x, x2, wp, bias, y, stat_part, act, nullptr, stream, VIAI_FORM_F32);
}
extern "C" int viai_conv2d_fwd_amax(const viai_conv2d* c, const float* x, const float* x2, const float* wp,
                                    const float* bias, float* y, float* stat_part, int act, const float* x_amax, void* stream) {
    return fwd_impl(c, x, x2, wp, bias, y, stat_part, act, x_amax, stream, x_amax != nullptr ? VIAI_FORM_AMAX : VIAI_FORM_F32);
}
// (ABI 13) the forward with x pre-split (P16 planes, scale from *x_amax): layers with VIAI_P16_OK_FWD_X in viai_conv2d_p16_ok
extern "C" int viai_conv2d_fwd_p16(const viai_conv2d* c, const float* x, const float* wp, const float* bias, float* y, float* stat_part,
                                   int act, const float* x_amax, void* stream) {
    if (x_amax == nullptr) return (int)hipErrorInvalidValue;
    return fwd_impl(c, x, nullptr, wp, bias, y, stat_part, act, x_amax, stream, VIAI_FORM_P16);
}

// ---- data gradient -------------------------------------------------------------------------------------------
static int dgrad_impl(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2, const float* amax, void* stream, int form) {
    if (!valid(c) || (c->C2 > 0) != (dx2 != nullptr)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    viai_tag_reset();
    ConvArgs a{};
    const ConvRoute r = route_dgrad(c, form, a);
    if (!r.ok) return (int)hipErrorInvalidValue;
    if (r.kernel == CK_DIRECT) {
        viai_tag_kernel(r.family);
        return kind_of(c) == K_CIN1 ? viai_cin1_dgrad(c, dy, wp, dx, st) : viai_cout1_dgrad(c, dy, wp, dx, st);
    }
    if (r.zero_fill) {
        size_t px = (size_t)c->N * c->IH * c->IW;
        if (hipMemsetAsync(dx, 0, px * c->C1 * sizeof(float), st) != hipSuccess) return (int)hipErrorInvalidValue;
        if (dx2 && hipMemsetAsync(dx2, 0, px * c->C2 * sizeof(float), st) != hipSuccess) return (int)hipErrorInvalidValue;
    }
    a.in = dy; a.wp = wp; a.out = dx; a.out2 = dx2;
    a.act = VIAI_ACT_NONE;
    a.amax = amax;
    if (r.fused) {
        int oh, ow; viai_conv2d_out_hw(c, &oh, &ow);
        a.g = ConvGeom{};
        a.g.N = c->N; a.g.IH = oh; a.g.IW = ow; a.g.OH = c->IH; a.g.OW = c->IW;
        a.M = c->N * (c->IH / 2) * (c->IW / 2);
        return launch_conv_kernel(r, a, st);
    }
    for (int a_ = 0; a_ < c->sh; ++a_)
        for (int b_ = 0; b_ < c->sw; ++b_) {
            // (one argument block for all classes: tap slots beyond ntaps keep the previous class's values, which no kernel reads)
            if (a_ + b_ > 0 && viai_geom_dgrad_class(c, a_, b_, &a.g) == 0) continue;        // (class (0, 0) is in a.g already; tapless: zero-filled above)
            if (a.g.SH <= 0 || a.g.SW <= 0 || a.g.ntaps == 0) continue;
            a.M = a.g.N * a.g.SH * a.g.SW;
            ConvRoute rc = r;                                 // strided: the tile instance follows the rows of the class
            if (c->sh * c->sw > 1) { rc.kernel = CK_NONE; if (r.bf3) pick_split_kernel(rc, a, r.halo, false, false, false); else pick_f32_kernel(rc, a); }
            int e = launch_conv_kernel(rc, a, st);
            if (e) return e;
        }
    return 0;
}
extern "C" int viai_conv2d_dgrad(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2, void* stream) {
    return dgrad_impl(c, dy, wp, dx, dx2, nullptr, stream, VIAI_FORM_F32);
}
// dy_amax: device float holding max |dy| (viai_bn_act_bwd_amax): the f16x2 operand scale is derived from it on the device
extern "C" int viai_conv2d_dgrad_f16(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2,
                                     const float* dy_amax, void* stream) {
    if (dy_amax == nullptr) return (int)hipErrorInvalidValue;
    return dgrad_impl(c, dy, wp, dx, dx2, dy_amax, stream, VIAI_FORM_AMAX);
}
// (ABI 13) viai_conv2d_dgrad_f16 with dy pre-split (P16 planes, scale from *dy_amax): layers with VIAI_P16_OK_DGRAD_DY
extern "C" int viai_conv2d_dgrad_f16_p16(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2,
                                         const float* dy_amax, void* stream) {
    if (dy_amax == nullptr) return (int)hipErrorInvalidValue;
    return dgrad_impl(c, dy, wp, dx, dx2, dy_amax, stream, VIAI_FORM_P16);
}

// ---- weight gradient -----------------------------------------------------------------------------------------
extern "C" size_t viai_conv2d_wgrad_ws_bytes(const viai_conv2d* c) {
    if (!valid(c)) return 0;
    WgradArgs a{};
    const ConvRoute r = route_wgrad(c, VIAI_FORM_F32, a);
    size_t ks = r.ksplit, fl;
    switch (kind_of(c)) {
    case K_CIN1: fl = viai_cin1_wgrad_ws_floats(c); break;
    case K_COUT1: fl = viai_cout1_wgrad_ws_floats(c); break;
    case K_RUN:
        if (r.f16 && (size_t)viai_conv_stem_wgrad_slabs(a.g) > ks) ks = viai_conv_stem_wgrad_slabs(a.g);
        fl = ks * viai_conv2d_packed_floats(c); break;
    default:                                                  // the workspace covers every form the layer can take, whatever VIAI_WGRAD_PATCH_S2 says
        if (f16x2_enabled() && bf3_enabled() && viai_wgrad_patch_cfg(a.g, c->Cout, c->C1, c->C2, false) != 0) {
            const size_t kp = viai_wgrad_patch_ksplit(a.g, c->Cout, c->C1, c->C2);
            if (kp > ks) ks = kp;
        }
        fl = ks * viai_conv2d_packed_floats(c);
    }
    // + column-sum partials for the bias gradient
    fl += (size_t)viai_colsum_blocks((long)a.M, c->Cout) * c->Cout;
    return fl * sizeof(float);
}

// f16x2 weight gradient: dy scaled on the device from dy_amax = max |dy|, x by the static activation scale or from x_amax; the layers of the
// f16x2 wgrad_bf3 kernel (> 32 channels on both sides), every layer an instance of the patch kernel takes, and the stem
extern "C" int viai_conv2d_wgrad_f16_ok(const viai_conv2d* c) {
    if (!valid(c)) return 0;
    WgradArgs a{};
    return route_wgrad(c, VIAI_FORM_F32, a).f16 ? 1 : 0;
}

// (ABI 13) which operands of this layer's f16x2 kernels may arrive pre-split (P16 planes, csrc/viai_bf3.h): a mask of VIAI_P16_OK_*
extern "C" int viai_conv2d_p16_ok(const viai_conv2d* c) {
    if (!valid(c) || kind_of(c) != K_IGEMM || !f16x2_enabled() || !bf3_enabled()) return 0;
    ConvArgs a{}, b{}; WgradArgs w{};
    return route_wgrad(c, VIAI_FORM_F32, w).p16 | route_fwd(c, VIAI_FORM_F32, a).p16 | route_dgrad(c, VIAI_FORM_F32, b).p16;
}

static int wgrad_impl(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                      float* ws, float* dw, float* db, int accumulate, const float* amax, const float* xmax, void* stream, int form) {
    if (!valid(c) || (c->C2 > 0) != (x2 != nullptr)) return (int)hipErrorInvalidValue;
    const int flags = (form & 3) == VIAI_FORM_P16 ? (form >> 2) : 0;
    if (((flags & VIAI_P16_DY) && db != nullptr) || ((flags & VIAI_P16_X) && xmax == nullptr)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    viai_tag_reset();
    WgradArgs a{};
    const ConvRoute r = route_wgrad(c, form, a);
    if (!r.ok) return (int)hipErrorInvalidValue;
    const int T = c->kh * c->kw, Cin = cin_of(c);
    a.x = x; a.x2 = kind_of(c) == K_RUN ? nullptr : x2; a.dy = dy; a.ws = ws; a.amax = amax; a.xmax = xmax;
    size_t used = (size_t)r.ksplit * viai_conv2d_packed_floats(c);
    int e = 0;
    viai_tag_kernel(r.family);
    switch (r.kernel) {
    case CK_DIRECT:
        if (kind_of(c) == K_CIN1) { e = viai_cin1_wgrad(c, x, dy, ws, dw, accumulate, st); used = viai_cin1_wgrad_ws_floats(c); }
        else { e = viai_cout1_wgrad(c, x, dy, ws, dw, accumulate, st); used = viai_cout1_wgrad_ws_floats(c); }
        break;
    case CK_WGRAD_STEM: e = viai_conv_stem_wgrad_launch(a, Cin, dw, accumulate, st); break;       // slabs + reduce in one call
    case CK_WGRAD_PATCH: e = viai_wgrad_patch_launch(a, st); break;
    case CK_WGRAD32: e = viai_wgrad32_launch(a, r.ksplit, st); break;
    case CK_WGRAD_BF3: e = viai_wgrad_bf3_launch(a, r.ksplit, st); break;
    default: e = viai_wgrad_mfma_launch(a, r.ksplit, st);
    }
    if (e) return e;
    if (kind_of(c) == K_RUN && r.kernel == CK_WGRAD_MFMA) {
        int total = c->Cout * Cin * T;
        VIAI_LAUNCH(wgrad_reduce_run_kernel, dim3((total + 255) / 256), dim3(256), 0, st, ws, dw, r.ksplit, c->Cout, Cin, c->kh, c->kw, accumulate);
        e = viai_launch_status();
    } else if (kind_of(c) == K_IGEMM) {
        if (c->transposed) e = viai_wgrad_reduce(ws, dw, r.ksplit, T, c->Cout, Cin, T, (long)c->Cout * T, accumulate, st);
        else e = viai_wgrad_reduce(ws, dw, r.ksplit, T, c->Cout, Cin, (long)Cin * T, T, accumulate, st);
    }
    if (e) return e;
    if (db != nullptr) e = viai_colsum(dy, a.M, c->Cout, ws + used, db, accumulate, stream);
    return e;
}
extern "C" int viai_conv2d_wgrad(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                                 float* ws, float* dw, float* db, int accumulate, void* stream) {
    return wgrad_impl(c, x, x2, dy, ws, dw, db, accumulate, nullptr, nullptr, stream, VIAI_FORM_F32);
}
extern "C" int viai_conv2d_wgrad_f16(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                                     float* ws, float* dw, float* db, int accumulate, const float* dy_amax, const float* x_amax, void* stream) {
    if (dy_amax == nullptr) return (int)hipErrorInvalidValue;
    return wgrad_impl(c, x, x2, dy, ws, dw, db, accumulate, dy_amax, x_amax, stream, VIAI_FORM_AMAX);
}
extern "C" int viai_conv2d_wgrad_f16_p16(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                                         float* ws, float* dw, float* db, int accumulate, const float* dy_amax, const float* x_amax, int flags, void* stream) {
    if (dy_amax == nullptr || flags < 0) return (int)hipErrorInvalidValue;
    return wgrad_impl(c, x, x2, dy, ws, dw, db, accumulate, dy_amax, x_amax, stream, flags ? (VIAI_FORM_P16 | (flags << 2)) : VIAI_FORM_AMAX);
}
