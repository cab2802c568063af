#!/usr/bin/env python
"""Times the MaskNet kernels (csrc/masknet.hip) at the Criteo shape - B = 65 536, F = 26, D = 16, parallel, 3 blocks,
H = 256, ratio 2 - with hipEvents after warm-up, 50 timed launches (min / median / mean), every launch on the next of
several buffer sets that together exceed the caches (more than 512 MB against 256 MB of Infinity Cache), beside the
comparator: the same arithmetic composed from torch ops in fp32 over the same inputs (layer_norm, the products, autograd
backward), the contenders taking turns in one process.  Each kernel is priced in algorithmic bytes against the 8 TB/s
HBM spec: group forward 4 B F D (1 + 2 N), group backward 4 B F D (2 + 3 N), row forward 8 B H, row backward 12 B H
(+ parameters).  Also MaskNetEngine.fwd_bwd, parallel and serial.  The shader clock the tools report is recorded.
    python tools/bench_masknet.py [--json out.json] [--kernels-only | --step-only]
`--kernels-only` launches nothing but the fused kernels, `--step-only` nothing but the engine's step (the runs to put
under rocprofv3 --kernel-trace --stats)."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as Fn

from recman_amd import engine as eng
from recman_amd import ops
from tools._bench import PEAK_HBM, alternate, criteo_like, emit, selected

ROTATE_BYTES = 512 << 20


def clock():
    """The shader clock as rocm-smi reports it while the GPU is busy (None when the tool is missing)."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln][:1] or None
    except Exception:  # noqa: BLE001
        return None


def _sets(per_set_bytes):
    return max(2, -(-ROTATE_BYTES // per_set_bytes))


def group(B, F, D, N, comparator=True):
    W = F * D
    S = _sets(4 * B * W * (1 + 2 * N))
    r = lambda *s: torch.randn(*s, device="cuda")  # noqa: E731
    gamma, beta = 1 + 0.5 * r(F, D), 0.3 * r(F, D)
    E = [r(B, F, D) for _ in range(S)]
    M = [[r(B, W) for _ in range(N)] for _ in range(S)]
    Y = [[torch.empty(B, W, device="cuda") for _ in range(N)] for _ in range(S)]
    dY = [[r(B, W) for _ in range(N)] for _ in range(S)]
    dM = [[torch.empty(B, W, device="cuda") for _ in range(N)] for _ in range(S)]
    d_rows, dg, db = torch.empty(B, F, D, device="cuda"), torch.empty(F, D, device="cuda"), torch.empty(F, D, device="cuda")
    ws = torch.empty(max(4, ops.masknet_group_bwd_workspace(B, F, D)), device="cuda")
    fwd = lambda i: ops.masknet_group_fwd(E[i % S], gamma, beta, M[i % S], Y[i % S])  # noqa: E731
    bwd = lambda i: ops.masknet_group_bwd(E[i % S], gamma, beta, M[i % S], dY[i % S], dM[i % S], d_rows, dg, db,  # noqa: E731
                                          ws)
    fns = [fwd, bwd]
    if comparator:
        gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def composed(i):
            e = E[i % S].detach().requires_grad_(True)
            ms = [m.detach().requires_grad_(True) for m in M[i % S]]
            V = (Fn.layer_norm(e, (D,), eps=1e-5) * gl + bl).view(B, W)
            ys = [m * V for m in ms]
            torch.autograd.backward(ys, dY[i % S])
            gl.grad = bl.grad = None

        fns.append(composed)
    ms = alternate(fns, indexed=True)  # fn(i) works on buffer set i
    fb, bb = 4.0 * (B * W * (1 + 2 * N) + 2 * W), 4.0 * (B * W * (2 + 3 * N) + 4 * W)
    rec = {"kernel": "group", "shape": dict(B=B, F=F, D=D, N=N, buffer_sets=S,
                                            tile=ops.masknet_group_tile(F, D, "tile"),
                                            cap=ops.masknet_group_tile(F, D, "cap")),
           "fwd_ms": ms[0], "bwd_ms": ms[1], "fwd_gb": round(fb / 1e9, 4), "bwd_gb": round(bb / 1e9, 4),
           "fwd_gb_s": round(fb / (ms[0]["median"] * 1e-3) / 1e9, 1),
           "bwd_gb_s": round(bb / (ms[1]["median"] * 1e-3) / 1e9, 1)}
    rec.update(fwd_peak_share=round(rec["fwd_gb_s"] * 1e9 / PEAK_HBM, 4),
               bwd_peak_share=round(rec["bwd_gb_s"] * 1e9 / PEAK_HBM, 4))
    if comparator:
        rec.update(composed_fwd_bwd_ms=ms[2],
                   ratio_composed_over_fused=round(ms[2]["median"] / (ms[0]["median"] + ms[1]["median"]), 2))
    return rec


def row(B, H, comparator=True):
    S = _sets(4 * B * H * 3)
    r = lambda *s: torch.randn(*s, device="cuda")  # noqa: E731
    gamma, beta = 1 + 0.5 * r(H), 0.3 * r(H)
    Z, dh = [r(B, H) for _ in range(S)], [r(B, H) for _ in range(S)]
    h, dZ = [torch.empty(B, H, device="cuda") for _ in range(S)], [torch.empty(B, H, device="cuda") for _ in range(S)]
    dg, db = torch.empty(H, device="cuda"), torch.empty(H, device="cuda")
    ws = torch.empty(max(4, ops.masknet_row_bwd_workspace(B, H)), device="cuda")
    fns = [lambda i: ops.masknet_row_fwd(Z[i % S], gamma, beta, h[i % S]),
           lambda i: ops.masknet_row_bwd(Z[i % S], gamma, beta, dh[i % S], dZ[i % S], dg, db, ws)]
    if comparator:
        gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def composed(i):
            z = Z[i % S].detach().requires_grad_(True)
            torch.relu(Fn.layer_norm(z, (H,), gl, bl, eps=1e-5)).backward(dh[i % S])
            gl.grad = bl.grad = None

        fns.append(composed)
    ms = alternate(fns, indexed=True)  # fn(i) works on buffer set i
    fb, bb = 4.0 * (2 * B * H + 2 * H), 4.0 * (3 * B * H + 4 * H)
    rec = {"kernel": "row", "shape": dict(B=B, H=H, buffer_sets=S, tile=ops.masknet_row_tile(H, "tile"),
                                          cap=ops.masknet_row_tile(H, "cap")),
           "fwd_ms": ms[0], "bwd_ms": ms[1], "fwd_gb": round(fb / 1e9, 4), "bwd_gb": round(bb / 1e9, 4),
           "fwd_gb_s": round(fb / (ms[0]["median"] * 1e-3) / 1e9, 1),
           "bwd_gb_s": round(bb / (ms[1]["median"] * 1e-3) / 1e9, 1)}
    rec.update(fwd_peak_share=round(rec["fwd_gb_s"] * 1e9 / PEAK_HBM, 4),
               bwd_peak_share=round(rec["bwd_gb_s"] * 1e9 / PEAK_HBM, 4))
    if comparator:
        rec.update(composed_fwd_bwd_ms=ms[2],
                   ratio_composed_over_fused=round(ms[2]["median"] / (ms[0]["median"] + ms[1]["median"]), 2))
    return rec


def step(order, B=65536, F=26, D=16, Dn=13, N=3, H=256, ratio=2.0, hidden=(128, 128)):
    """MaskNetEngine.fwd_bwd, hashed ids over 26 x 40000 rows."""
    spec, idx, dense, y = criteo_like(B, F, Dn)
    e = eng.MaskNetEngine(spec, D, dict(block_order=order, num_blocks=N, block_hidden_units=H, reduction_ratio=ratio,
                                        deep_hidden_units=tuple(hidden)))
    eng.init_reference(e)
    return alternate([lambda: e.fwd_bwd(idx, dense, y)], n=20, warm=3)[0]


if __name__ == "__main__":
    res = selected(lambda comparator: [group(65536, 26, 16, 3, comparator=comparator),
                                       row(65536, 256, comparator=comparator)],
                   lambda: {f"masknet_{o}_fwd_bwd_ms": step(o) for o in ("parallel", "serial")})
    res["clock"] = clock()
    emit(res)
