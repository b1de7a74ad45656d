"""The weight images of the pipelined WaveNet synthesis kernel (csrc/wavenet_pipe.hip), checked without a GPU: a numpy restatement of what a
stage's lanes do with the images (register image: wave, register index, lane; LDS rows; conditioning rows) must give the layer's plain formulas
(wavenet_vocoder/modules.py:162-210 in the fused form of csrc/wavenet.hip) -- i.e. the host packing and the kernel's index arithmetic agree."""
import numpy as np
import torch

from viai_amd import wavenet_synth as WN

NL, NCU, NW, GW, BW, C, H, S, CIN = 24, 10, 8, 7, 10, 512, 256, 256, 80
R5 = np.float64(0.5) ** 0.5


def test_pipe_images_reproduce_the_fused_stage_formulas():
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)
    w_stage = [rnd(2 * H, 3 * C + (H if l else 0)) for l in range(NL)]
    b_stage = [rnd(2 * H) for _ in range(NL)]
    w_c = [rnd(2 * H, CIN) for _ in range(NL)]
    w_out, b_out = [rnd(C, H) for _ in range(NL)], [rnd(C) for _ in range(NL)]
    w_skip, b_skip = [rnd(S, H) for _ in range(NL)], [rnd(S) for _ in range(NL)]
    w1, b1, w2, b2 = rnd(S, S), rnd(S), rnd(30, S), rnd(30)
    f = lambda ts: [t.float() for t in ts]
    wreg, wcond, wlds, bias, head_w, head_b = WN._pipe_images(f(w_stage), f(b_stage), f(w_c), f(w_out), f(b_out), f(w_skip), f(b_skip),
                                                              w1.float(), b1.float(), w2.float(), b2.float(), "cpu")
    assert tuple(wreg.shape) == (NL, NCU, NW, 156, 64) and tuple(wcond.shape) == (NL, NCU, 64, CIN)
    assert tuple(wlds.shape) == (NL, NCU, 130, 260) and tuple(bias.shape) == (NL, NCU, 136) and tuple(head_w.shape) == (544, 256)
    wreg, wcond, wlds, bias = (t.double().numpy() for t in (wreg, wcond, wlds, bias))
    lane = np.arange(64)
    for l in (0, 1, 7, 23):
        x2, x1, xc, cnd = (rnd(C).numpy(), rnd(C).numpy(), rnd(C).numpy(), rnd(CIN).numpy())       # x_l(t-2d), x_l(t-d), x_{l-1}(t) (l = 0: x_0(t)), c_t
        zin, skin = rnd(H).numpy(), rnd(S).numpy()
        xpre = np.concatenate((x2, x1))
        z_out, x_out, s_out = np.zeros(H), np.zeros(C), np.zeros(S)
        for j in range(NCU):
            g_, cg = lane // 16, lane % 16
            pg, pb = np.zeros((NW, 52)), np.zeros((NW, 80))
            for wave in range(NW):
                for i in range(13):                        # lane (g, cg): rows 13 g + i; reduced over the 16 lanes of a row group
                    acc = np.zeros(64)
                    for m in range(2):                     # past taps: register 8 i + 4 m + e <-> column 128 wave + 64 m + 4 cg + e
                        for e in range(4):
                            acc += wreg[l, j, wave, 8 * i + 4 * m + e] * xpre[128 * wave + 64 * m + 4 * cg + e]
                    for e in range(4):                     # current tap: register 104 + 4 i + e <-> column 64 wave + 4 cg + e
                        acc += wreg[l, j, wave, 104 + 4 * i + e] * xc[64 * wave + 4 * cg + e]
                    for grp in range(4):
                        pg[wave, 13 * grp + i] += acc[g_ == grp].sum()
                if l > 0:                                  # LDS rows: lane = row, the wave's 32 columns of z
                    zc = zin[32 * wave:32 * wave + 32]
                    for r in range(52):
                        pg[wave, r] += (wlds[l, j, r, 32 * wave:32 * wave + 32] * zc).sum()
                    for q in range(78):
                        pb[wave, q] = (wlds[l, j, 52 + q, 32 * wave:32 * wave + 32] * zc).sum()
            gsum = np.concatenate((pg.sum(0), np.zeros(4)))
            bres = pb.sum(0)
            assert np.all(wlds[l, j, :, 256:] == 0)
            cpart = (wcond[l, j] * cnd[None, :]).sum(1)
            for k in range(26):
                h = 26 * j + k
                if h < H:
                    va, vg = gsum[k] + bias[l, j, k] + cpart[k], gsum[26 + k] + bias[l, j, 26 + k] + cpart[26 + k]
                    z_out[h] = np.tanh(va) / (1 + np.exp(-vg))
            for k in range(52):
                c = 52 * j + k
                if c < C:
                    x_out[c] = xc[c] if l == 0 else (bres[k] + bias[l, j, 56 + k] + xc[c]) * R5
            for k in range(26):
                si = 26 * j + k
                if si < S:
                    s_out[si] = 0.0 if l == 0 else (bres[52 + k] + bias[l, j, 56 + 52 + k] if l == 1 else (skin[si] + bres[52 + k] + bias[l, j, 56 + 52 + k]) * R5)
        # the plain formulas (fused chain form, csrc/wavenet.hip wn_stage_kernel)
        ws, wc = w_stage[l].numpy(), w_c[l].numpy()
        col = np.concatenate((x2, x1, xc, zin)) if l > 0 else np.concatenate((x2, x1, xc))
        gate = ws @ col + b_stage[l].numpy() + wc @ cnd
        z_ref = np.tanh(gate[:H]) / (1 + np.exp(-gate[H:]))
        assert np.abs(z_out - z_ref).max() < 1e-5
        if l == 0:
            assert np.array_equal(x_out, xc)
        else:
            x_ref = (w_out[l - 1].numpy() @ zin + b_out[l - 1].numpy() + xc) * R5
            sk = w_skip[l - 1].numpy() @ zin + b_skip[l - 1].numpy()
            s_ref = sk if l == 1 else (skin + sk) * R5
            assert np.abs(x_out - x_ref).max() < 1e-5 and np.abs(s_out - s_ref).max() < 1e-5
    # head rows
    hw, hb = head_w.double().numpy(), head_b.double().numpy()
    assert np.allclose(hw[:256], w_skip[NL - 1].numpy(), atol=1e-6) and np.allclose(hw[256:512], w1.numpy(), atol=1e-6)
    assert np.allclose(hw[512:542], w2.numpy(), atol=1e-6) and np.all(hw[542:] == 0) and np.allclose(hb[512:542], b2.numpy(), atol=1e-6)
