#!/usr/bin/env python3
"""Record the conv dispatch table of the built library on a machine WITHOUT a GPU.

Every query of the conv family is host code, and a launch entry point called without a device sets its kernel-family tag
(viai_conv2d_last_kernel) and then fails with hipErrorNoDevice before it touches an operand.  So the complete decision table --
which kernel, weight image, BatchNorm partial geometry and P16 mask a descriptor gets -- can be written down and compared
between two builds byte for byte:

    python3 tools/conv_routes.py --record OUT.json [--lib PATH/libviai_hip.so]      # full sweep (about 75 k descriptors)
    python3 tools/conv_routes.py --record OUT.json --descs FILE.json                # only the descriptors listed in FILE
    python3 tools/conv_routes.py --wavenet --merge tests/golden/conv_routes.json    # append the WaveNet Conv1d layers not yet in the table
    python3 tools/conv_routes.py --check-route                                      # viai_conv2d_route == the tag of the launch, every row
    python3 tools/conv_routes.py --time 20 --descs FILE.json [--lib ...]            # host microseconds per entry-point call, no device

The launch part passes null operands: it REFUSES to run when a GPU is present.

Row layout (all integers unless noted; a descriptor has 13 fields, or 17 where the layer is dilated or padded on one side only:
FIELDS then dh, dw, ph2, pw2 as include/viai_hip.h defines them):
    [desc(13 | 17), stat_geom(rc, nblk, rows), stat_tiles(rc, th, tw), packed_floats, wgrad_ws_bytes,
     fwd_f16_ok, dgrad_f16_ok, wgrad_f16_ok, p16_ok, pack_job x 3 (rc, frag, n_out, k_in, s_no, s_ki, nblk),
     launch x 9 (rc, launches, family)]
launch order = LAUNCHES below; (pass, form) of each for viai_conv2d_route is PASS_FORM.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("N", "IH", "IW", "C1", "C2", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "transposed")
LAUNCHES = ("fwd", "fwd_amax", "fwd_p16", "dgrad", "dgrad_f16", "dgrad_f16_p16", "wgrad", "wgrad_f16", "wgrad_f16_p16")
P16_DY, P16_X = 1, 2
FORM_F32, FORM_AMAX, FORM_P16 = 0, 1, 2


def wgrad_p16_flags(d):
    """flags of the recorded viai_conv2d_wgrad_f16_p16 call: both operands pre-split where the layer has one source"""
    return (P16_DY | P16_X) if d[4] == 0 else P16_DY


def tapless_class(d):
    """a parity class of the (plain, undilated) data gradient that no tap reaches, e.g. 1 x 1 stride 2"""
    kh, kw, sh, sw, ph, pw = d[6:12]
    rows = {(r - ph) % sh for r in range(kh)}
    cols = {(s - pw) % sw for s in range(kw)}
    return not d[12] and (len(rows) < min(sh, d[1]) or len(cols) < min(sw, d[2]))


def pass_form(i, d):
    """(pass, form) arguments of viai_conv2d_route for launch entry i of LAUNCHES"""
    p, f = divmod(i, 3)
    if p == 2 and f == FORM_P16:
        f |= wgrad_p16_flags(d) << 2
    return p, f


def desc17(d):
    """the 17 fields of viai_conv2d from a row's descriptor: 13 fields mean no dilation and symmetric padding"""
    d = tuple(d)
    if len(d) == 13:
        return d + (0, 0, -1, -1)
    assert len(d) == 17, d
    return d


# The Conv1d layers of one teacher-forced WaveNet training step (viai_amd/wavenet.py: conv1d_apply): kh = 1 on (B, 1, T, C) tensors, the
# k = 3 layer dilated by dw = 2^i and padded on the left only (pw = 2 dw, pw2 = 0), every other layer 1 x 1.  (name, Cin, Cout, k) of every
# layer of each network width; head2 is the 30-channel output layer as the step runs it, padded to 32 rows (WaveNet.forward_nhwc), and
# head2_unpadded the same layer without the padding (a forward route only).  Layers of one network, or of two, that share a descriptor
# (deep: out and skip; 32 -> 32 1 x 1 in small and deep) are recorded once: wavenet_descs() drops the repeats.
WAVENET_LAYERS = {
    "full": (("conv", 512, 512, 3), ("cond", 80, 512, 1), ("out", 256, 512, 1), ("skip", 256, 256, 1), ("head1", 256, 256, 1),
             ("head2", 256, 32, 1), ("head2_unpadded", 256, 30, 1)),
    "small": (("conv", 64, 64, 3), ("cond", 80, 64, 1), ("out", 32, 64, 1), ("skip", 32, 32, 1), ("head1", 32, 32, 1),
              ("head2", 32, 32, 1), ("head2_unpadded", 32, 30, 1)),
    "deep": (("conv", 32, 32, 3), ("cond", 80, 32, 1), ("out", 16, 32, 1), ("skip", 16, 32, 1), ("head1", 32, 32, 1),
             ("head2", 32, 32, 1), ("head2_unpadded", 32, 30, 1)),
}
WAVENET_DILATIONS = (1, 2, 4, 8, 16, 32)


def wavenet_desc(N, T, cin, cout, k, d=1, causal=True):
    """17-field descriptor of a WaveNet Conv1d on (N, 1, T, cin): causal = left padding (k - 1) d, else (k - 1) / 2 * d on both sides"""
    if k == 1:
        return (N, 1, T, cin, 0, cout, 1, 1, 1, 1, 0, 0, 0, 1, 1, -1, -1)
    if causal:
        return (N, 1, T, cin, 0, cout, 1, k, 1, 1, 0, (k - 1) * d, 0, 1, d, -1, 0)
    return (N, 1, T, cin, 0, cout, 1, k, 1, 1, 0, (k - 1) // 2 * d, 0, 1, d, -1, -1)


def wavenet_descs():
    """the layers of WAVENET_LAYERS at N = 2: T = 8192 (a training batch of the reference) and T = 64 (the golden's), every dilation of a
    stack for the k = 3 layer"""
    out = []
    for T in (8192, 64):
        for layers in WAVENET_LAYERS.values():
            for _name, cin, cout, k in layers:
                for d in (WAVENET_DILATIONS if k > 1 else (1,)):
                    desc = wavenet_desc(2, T, cin, cout, k, d)
                    if desc not in out:
                        out.append(desc)
    return out


def sweep():
    sizes = [(256, 256), (128, 128), (64, 32), (16, 32), (2, 16), (56, 56), (28, 28), (14, 14), (7, 7), (80, 208), (40, 104), (20, 26),
             (224, 224), (112, 112), (32, 64)]
    windows = [(3, 3, 1, 1), (1, 1, 0, 0), (1, 4, 0, 1), (1, 3, 0, 1), (5, 5, 2, 2), (7, 7, 3, 3)]
    for N, (IH, IW), C1, two, Cout, (kh, kw, ph, pw), (sh, sw), tr in itertools.product(
            (1, 2, 16, 1024), sizes, (1, 3, 16, 32, 64, 128, 256, 512), (0, 1), (1, 32, 64, 128, 256, 512), windows,
            ((1, 1), (2, 2), (2, 1)), (0, 1)):
        yield (N, IH, IW, C1, C1 if two else 0, Cout, kh, kw, sh, sw, ph, pw, tr)


def gpu_present(lib):
    import torch
    if torch.cuda.is_available():
        return True
    try:
        hip = C.CDLL("libamdhip64.so")
        n = C.c_int(0)
        return hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def open_lib(path):
    from viai_amd import _lib                      # (imports torch first: the library binds to torch's HIP runtime)
    lib = C.CDLL(path or _lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, _lib


def record(lib, _lib, descs, launches=True, route=False):
    D, J = _lib.Conv2dDesc, _lib.PackJob
    dummy = (C.c_float * 4)()
    amax = C.cast(dummy, C.c_void_p)
    i1, i2 = C.c_int(), C.c_int()
    buf = C.create_string_buffer(64)
    rows, bad = [], 0
    reset = D(1, 16, 16, 3, 0, 64, 7, 7, 2, 2, 3, 3, 0, 0, 0, -1, -1)
    assert lib.viai_conv2d_dgrad(C.byref(reset), None, None, None, None, None) == 1 and lib.viai_conv2d_last_kernel(buf, 64) == 0
    for d in descs:
        c = D(*desc17(d))
        if lib.viai_conv2d_stat_geom(C.byref(c), C.byref(i1), C.byref(i2)) != 0:
            continue                                # not a valid descriptor
        row = [list(d), [0, i1.value, i2.value]]
        rc = lib.viai_conv2d_stat_tiles(C.byref(c), C.byref(i1), C.byref(i2))
        row.append([rc, i1.value, i2.value])
        row += [lib.viai_conv2d_packed_floats(C.byref(c)), lib.viai_conv2d_wgrad_ws_bytes(C.byref(c)),
                lib.viai_conv2d_fwd_f16_ok(C.byref(c)), lib.viai_conv2d_dgrad_f16_ok(C.byref(c)),
                lib.viai_conv2d_wgrad_f16_ok(C.byref(c)), lib.viai_conv2d_p16_ok(C.byref(c))]
        for dg in (0, 1, 2):
            j = J()
            rc = lib.viai_conv2d_pack_job(C.byref(c), dg, None, None, C.byref(j))
            row.append([rc] + ([j.frag, j.n_out, j.k_in, j.s_no, j.s_ki, j.nblk] if rc == 0 else [0] * 6))
        if launches and not (d[3] + d[4] == 1 and d[5] < 4):      # (Cin = 1 with Cout < 4 once divided by zero in the weight gradient)
            two = amax if d[4] > 0 else None        # second source / destination: never dereferenced without a device
            cp = C.byref(c)
            calls = (
                lambda: lib.viai_conv2d_fwd(cp, None, two, None, None, None, None, 0, None),
                lambda: lib.viai_conv2d_fwd_amax(cp, None, two, None, None, None, None, 0, amax, None),
                lambda: lib.viai_conv2d_fwd_p16(cp, None, None, None, None, None, 0, amax, None),
                lambda: lib.viai_conv2d_dgrad(cp, None, None, None, two, None),
                lambda: lib.viai_conv2d_dgrad_f16(cp, None, None, None, two, amax, None),
                lambda: lib.viai_conv2d_dgrad_f16_p16(cp, None, None, None, two, amax, None),
                lambda: lib.viai_conv2d_wgrad(cp, None, two, None, None, None, None, 0, None),
                lambda: lib.viai_conv2d_wgrad_f16(cp, None, two, None, None, None, None, 0, amax, amax, None),
                lambda: lib.viai_conv2d_wgrad_f16_p16(cp, None, two, None, None, None, None, 0, amax, amax, wgrad_p16_flags(d), None),
            )
            for i, call in enumerate(calls):
                lib.viai_conv2d_dgrad(C.byref(reset), None, None, None, None, None)        # an image-input layer has no data gradient: clears the tag
                rc = call()
                n = lib.viai_conv2d_last_kernel(buf, 64)
                fam = buf.value.decode()
                row.append([rc, n, fam])
                if route:
                    p, f = pass_form(i, d)
                    rn = lib.viai_conv2d_route(cp, p, f, buf, 64)
                    rfam = buf.value.decode()
                    # a per-class data gradient stops at its first launch without a device: the tag then counts one launch;
                    # and one with a tapless parity class fails at the zero-fill before it chooses anything: nothing to compare
                    # (the route names the LAST class's kernel, whose tile instance may differ from the first's)
                    same = (rfam == fam and rn == n) or (p == 1 and n == 1 and rn > 1 and d[8] * d[9] > 1)
                    if p == 1 and rc == 1 and n == 0 and tapless_class(d):
                        same = True
                    if not same:
                        bad += 1
                        if bad <= 20:
                            print("route mismatch", d, LAUNCHES[i], "launch:", (rc, n, fam), "route:", (rn, rfam))
        rows.append(row)
    return rows, bad


def time_calls(lib, _lib, descs, rounds):
    """host time per call (microseconds, best of `rounds` passes over `descs`) of each launch entry point up to its failed launch, and of
    the queries: the dispatch cost that is left when the device is taken away"""
    import time
    D = _lib.Conv2dDesc
    dummy = (C.c_float * 4)()
    amax = C.cast(dummy, C.c_void_p)
    i1, i2 = C.c_int(), C.c_int()
    cs = [D(*desc17(d)) for d in descs]
    cs = [(c, C.byref(c), amax if c.C2 > 0 else None, wgrad_p16_flags((0, 0, 0, c.C1, c.C2))) for c in cs
          if lib.viai_conv2d_stat_geom(C.byref(c), C.byref(i1), C.byref(i2)) == 0 and not (c.C1 + c.C2 == 1 and c.Cout < 4)]
    calls = {
        "fwd": lambda c, cp, two, fl: lib.viai_conv2d_fwd(cp, None, two, None, None, None, None, 0, None),
        "fwd_amax": lambda c, cp, two, fl: lib.viai_conv2d_fwd_amax(cp, None, two, None, None, None, None, 0, amax, None),
        "fwd_p16": lambda c, cp, two, fl: lib.viai_conv2d_fwd_p16(cp, None, None, None, None, None, 0, amax, None),
        "dgrad": lambda c, cp, two, fl: lib.viai_conv2d_dgrad(cp, None, None, None, two, None),
        "dgrad_f16": lambda c, cp, two, fl: lib.viai_conv2d_dgrad_f16(cp, None, None, None, two, amax, None),
        "dgrad_f16_p16": lambda c, cp, two, fl: lib.viai_conv2d_dgrad_f16_p16(cp, None, None, None, two, amax, None),
        "wgrad": lambda c, cp, two, fl: lib.viai_conv2d_wgrad(cp, None, two, None, None, None, None, 0, None),
        "wgrad_f16": lambda c, cp, two, fl: lib.viai_conv2d_wgrad_f16(cp, None, two, None, None, None, None, 0, amax, amax, None),
        "wgrad_f16_p16": lambda c, cp, two, fl: lib.viai_conv2d_wgrad_f16_p16(cp, None, two, None, None, None, None, 0, amax, amax, fl, None),
        "stat_geom": lambda c, cp, two, fl: lib.viai_conv2d_stat_geom(cp, C.byref(i1), C.byref(i2)),
        "p16_ok": lambda c, cp, two, fl: lib.viai_conv2d_p16_ok(cp),
        "wgrad_ws_bytes": lambda c, cp, two, fl: lib.viai_conv2d_wgrad_ws_bytes(cp),
        "(empty call)": lambda c, cp, two, fl: lib.viai_abi_version(),
    }
    out = {}
    for name, f in calls.items():
        best = None
        for _ in range(rounds):
            t0 = time.perf_counter()
            for c, cp, two, fl in cs:
                f(c, cp, two, fl)
            dt = (time.perf_counter() - t0) * 1e6 / len(cs)
            best = dt if best is None or dt < best else best
        out[name] = round(best, 3)
    return len(cs), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, metavar="ROUNDS", default=0, help="time the entry points and queries (best of ROUNDS passes)")
    ap.add_argument("--record", metavar="OUT.json")
    ap.add_argument("--check-route", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--descs", default=None, help="JSON list of 13- or 17-integer descriptors (default: the sweep)")
    ap.add_argument("--wavenet", action="store_true", help="the descriptors of wavenet_descs() instead of the sweep")
    ap.add_argument("--merge", metavar="TABLE.json", help="append the recorded rows whose descriptor TABLE does not hold yet; its rows stay as they are")
    a = ap.parse_args()
    lib, _lib = open_lib(a.lib)
    if gpu_present(lib):
        sys.exit("conv_routes.py: a GPU is present; the launch entry points would dereference the null operands. Not run.")
    descs = [tuple(x) for x in json.load(open(a.descs))] if a.descs else wavenet_descs() if a.wavenet else sweep()
    if a.time:
        n, t = time_calls(lib, _lib, list(descs), a.time)
        print("%d descriptors, us per call: %s" % (n, json.dumps(t)))
        return
    rows, bad = record(lib, _lib, descs, route=a.check_route)
    fams = sorted({r[-1 - k][2] for r in rows if len(r) > 15 for k in range(9)} - {""})
    print("%d descriptors, %d kernel families: %s" % (len(rows), len(fams), " ".join(fams)))
    out = a.record
    if a.merge:
        old = json.load(open(a.merge))
        have = {tuple(r[0]) for r in old}
        new = [r for r in rows if tuple(r[0]) not in have]
        print("%s: %d rows, %d appended" % (a.merge, len(old), len(new)))
        rows, out = old + new, a.merge
    if out:
        with open(out, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    if a.check_route:
        print("route mismatches: %d" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
