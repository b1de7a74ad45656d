"""Shared by the optical-flow tests: the rule of include/viai_hip.h ("optical flow") restated in fp64 numpy, written from the header's text and
not from the C++, and the texture generator whose true flow is known exactly.  Nothing here needs the library or a GPU."""
import numpy as np

QUICK = dict(scales=3, warps=2, iterations=7)          # what the tests use unless they say otherwise
DEFAULTS = dict(tau=0.25, lam=0.15, theta=0.3, scales=5, warps=5, iterations=30)


# ----------------------------------------------------------------------------- textures with a known flow
def texture(N, H, W, shift, seed=0, waves=5):
    """(N, H, W) uint8: a sum of `waves` sinusoids with wavelengths 8 .. 40 px around 127.5, frame n evaluated analytically at
    (x - n dx, y - n dy) and then rounded, so the content moves by exactly shift = (dx, dy) pixels per frame"""
    r = np.random.RandomState(seed)
    lam = r.uniform(8.0, 40.0, waves)
    ang = r.uniform(0.0, np.pi, waves)
    ph = r.uniform(0.0, 2 * np.pi, waves)
    amp = r.uniform(0.5, 1.0, waves)
    amp *= 100.0 / amp.sum()
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((N, H, W), dtype=np.uint8)
    for n in range(N):
        xs, ys = x - n * shift[0], y - n * shift[1]
        val = np.full((H, W), 127.5)
        for k in range(waves):
            val += amp[k] * np.sin(2 * np.pi * (xs * np.cos(ang[k]) + ys * np.sin(ang[k])) / lam[k] + ph[k])
        out[n] = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    return out


def rgb_of(grey, seed=0):
    """(N, H, W, 3) uint8 whose channels differ (so that a channel mix-up shows) and whose grey value follows the texture"""
    r = np.random.RandomState(seed)
    g = grey.astype(np.int32)
    return np.stack([np.clip(g + r.randint(-20, 21, g.shape), 0, 255), g, np.clip(g + r.randint(-20, 21, g.shape), 0, 255)], axis=-1).astype(np.uint8)


# ----------------------------------------------------------------------------- the rule in fp64
def grey_rule(frames, bgr=False):
    f = np.asarray(frames)
    if f.ndim == 3 or f.shape[3] == 1:
        return f.reshape(f.shape[:3]).astype(np.float64)
    f = f.astype(np.int64)
    r, b = (f[..., 2], f[..., 0]) if bgr else (f[..., 0], f[..., 2])
    return ((4899 * r + 9617 * f[..., 1] + 1868 * b + 8192) >> 14).astype(np.float64)


def level_shapes(H, W, scales):
    out = [(H, W)]
    while len(out) < scales:
        h, w = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if h < 16 or w < 16:
            break
        out.append((h, w))
    return out


_TAPS = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def down_rule(a):
    h, w = a.shape
    hd, wd = (h + 1) // 2, (w + 1) // 2
    rows = 0.0
    for j, t in enumerate(_TAPS):                                         # rows first: along x on every source row
        rows = rows + t * a[:, np.clip(2 * np.arange(wd) - 2 + j, 0, w - 1)]
    out = 0.0
    for j, t in enumerate(_TAPS):                                         # then along y
        out = out + t * rows[np.clip(2 * np.arange(hd) - 2 + j, 0, h - 1), :]
    return out


def bilinear_rule(A, cx, cy):
    h, w = A.shape
    cx = np.where(cx >= 0, np.minimum(cx, w - 1), 0.0)                    # a NaN fails `>= 0` and lands on 0
    cy = np.where(cy >= 0, np.minimum(cy, h - 1), 0.0)
    x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = cx - x0, cy - y0
    return (1 - ay) * ((1 - ax) * A[y0, x0] + ax * A[y0, x1]) + ay * ((1 - ax) * A[y1, x0] + ax * A[y1, x1])


def central_rule(I):
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    Ix = 0.5 * (I[:, np.minimum(xs + 1, w - 1)] - I[:, np.maximum(xs - 1, 0)])
    Iy = 0.5 * (I[np.minimum(ys + 1, h - 1), :] - I[np.maximum(ys - 1, 0), :])
    return Ix, Iy


def up_rule(uc, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return 2.0 * bilinear_rule(uc, (x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5)


def back_rule(p, axis):
    """the backward difference of the divergence along `axis`"""
    p = np.moveaxis(p, axis, 0)
    d = np.zeros_like(p)
    if p.shape[0] > 1:
        d[0] = p[0]
        d[1:-1] = p[1:-1] - p[:-2]
        d[-1] = -p[-2]
    return np.moveaxis(d, 0, axis)


def fwd_rule(u, axis):
    u = np.moveaxis(u, axis, 0)
    d = np.zeros_like(u)
    d[:-1] = u[1:] - u[:-1]
    return np.moveaxis(d, 0, axis)


def tvl1_rule(frames, bgr=False, tau=0.25, lam=0.15, theta=0.3, scales=5, warps=5, iterations=30):
    """(N - 1, 2, H, W) float64.  The three real parameters are the fp32 numbers the library receives."""
    tau, lam, theta = (float(np.float32(v)) for v in (tau, lam, theta))
    g = grey_rule(frames, bgr)
    N, H, W = g.shape
    shapes = level_shapes(H, W, scales)
    pyr = []
    for n in range(N):
        lv = [g[n]]
        for _ in shapes[1:]:
            lv.append(down_rule(lv[-1]))
        pyr.append(lv)
    lt, taut = lam * theta, tau / theta
    flow = np.empty((N - 1, 2, H, W))
    for n in range(N - 1):
        u = v = None
        for k in range(len(shapes) - 1, -1, -1):
            h, w = shapes[k]
            I0, I1 = pyr[n][k], pyr[n + 1][k]
            I1x, I1y = central_rule(I1)
            if u is None:
                u, v = np.zeros((h, w)), np.zeros((h, w))
            else:
                u, v = up_rule(u, h, w), up_rule(v, h, w)
            p11, p12, p21, p22 = (np.zeros((h, w)) for _ in range(4))
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            for _ in range(warps):
                I1w, wx, wy = (bilinear_rule(A, x + u, y + v) for A in (I1, I1x, I1y))
                grad = wx * wx + wy * wy
                rho_c = I1w - wx * u - wy * v - I0
                safe = np.where(grad > 1e-10, grad, 1.0)
                for _ in range(iterations):
                    rho = rho_c + wx * u + wy * v
                    f = np.where(rho < -lt * grad, lt, np.where(rho > lt * grad, -lt, np.where(grad > 1e-10, -rho / safe, 0.0)))
                    u = (u + f * wx) + theta * (back_rule(p11, 1) + back_rule(p12, 0))
                    v = (v + f * wy) + theta * (back_rule(p21, 1) + back_rule(p22, 0))
                    ux, uy, vx, vy = fwd_rule(u, 1), fwd_rule(u, 0), fwd_rule(v, 1), fwd_rule(v, 0)
                    du, dv = 1 + taut * np.sqrt(ux * ux + uy * uy), 1 + taut * np.sqrt(vx * vx + vy * vy)
                    p11, p12 = (p11 + taut * ux) / du, (p12 + taut * uy) / du
                    p21, p22 = (p21 + taut * vx) / dv, (p22 + taut * vy) / dv
        flow[n, 0], flow[n, 1] = u, v
    return flow


def encode_rule(flow, bound=20.0, pad_last=True):
    """the encoding in the same fp32 operations: exact"""
    f, b = np.asarray(flow, dtype=np.float32), np.float32(bound)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.float32(255) * (f + b) / (np.float32(2) * b))      # numpy rounds every fp32 operation once; rint is half-to-even
        q = np.where(f > b, np.float32(255), q)
        q = np.where(f >= -b, q, np.float32(0))                           # below -bound, and a NaN
    q = np.minimum(q, 255).astype(np.uint8)
    if pad_last:
        q = np.concatenate([q, q[-1:]], axis=0)
    return np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])


def epe_interior(flow, shift, border=8):
    """mean end-point error of one (2, H, W) map against a constant true flow, an 8-px border left out"""
    du, dv = flow[0] - shift[0], flow[1] - shift[1]
    return float(np.sqrt(du * du + dv * dv)[border:-border, border:-border].mean())
