"""CPU checks of tests/mlp_ref.py, the float64 references of the skinny-MLP kernels (no GPU):
the stage functions, composed end to end, against an autograd restatement of the whole model and against the oracle's
DNN; and a torch fp32 emulation of every stage against the bounds the GPU module applies to the kernels
(front_refs.sum_bound with the n each stage states) - the reference alone must sit inside them, over every element, at
the GPU module's own shapes."""
import pytest
import torch

from oracle import th_layers as T
from tests import front_refs as R
from tests import mlp_cases as MC
from tests import mlp_ref as M
from tests.cases import make_case

F32, F64 = torch.float32, torch.float64


def _rel(got, want, what, tol=1e-12):
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1e-300, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= tol * scale, f"{what}: {err:.3e} (scale {scale:.3e})"


def _compose(p, act, y, task, *, D=0, lin_w=None, lin_w0=None, extra=None, coef_extra=1.0, grad_scale=1.0):
    """The stage functions chained the way the GPU module chains them (coef_mlp = 1, the only value a tail takes)."""
    xe, xd, Ws, bs = p["xe"], p["xd"], p["Ws"], p["bs"]
    x = xe if xd is None else torch.cat([xe, xd], 1)
    NL, B, FD = len(Ws), xe.shape[0], xe.shape[1]
    h = []
    for l in range(NL):
        h.append(M.layer_ref(x if l == 0 else h[l - 1], Ws[l], bs[l], act)[0])
    dnn = M.logit_ref(h[-1], p["w_out"], p["w0"])[0]
    branches = []
    S = None
    if lin_w is not None:
        branches.append((xd.to(F64) @ lin_w.to(F64) + lin_w0.to(F64), 1.0))
    if D:
        E = xe.to(F64).reshape(B, FD // D, D)
        S = E.sum(1)
        branches.append((0.5 * (S.square() - E.square().sum(1)).sum(1), 1.0))
    if extra is not None:
        branches.append((extra, coef_extra))
    head = M.head_ref(dnn, branches, 1.0, y, task, grad_scale)
    g = head["dlogit"]
    dh = [None] * NL
    dh[NL - 1] = M.dh_last_ref(g, p["w_out"], h[-1], act)[0]
    for l in range(NL - 1, 0, -1):
        dh[l - 1] = M.dh_prev_ref(dh[l], Ws[l], h[l - 1], act)[0]
    out = dict(h=h, dnn=dnn, z=head["logit"], pred=head["pred"], loss=head["loss"], g=g,
               xe=M.d_rows_ref(dh[0], Ws[0], FD, g, S, xe if D else None)[0],
               W=[M.dW0_ref(x, dh[0])[0]] + [M.dW_ref(h[l - 1], dh[l])[0] for l in range(1, NL)],
               b=[M.db_ref(d)[0] for d in dh], w_out=M.d_w_out_ref(h[-1], g)[0], w0=M.sum_g_ref(g)[0],
               lin_w=None if lin_w is None else M.d_xd_wsum_ref(xd, g)[0], lin_w0=M.sum_g_ref(g)[0])
    return out


SMALL = [  # FD, Dn, B, hidden, D (0: no FM term), linear term, extra branch coefficient (None: no branch)
    (8, 2, 5, (3, 2), 4, True, None),
    (12, 0, 9, (4,), 0, False, -0.5),
    (16, 3, 7, (5, 6, 3), 8, True, None),
    (0, 4, 6, (3, 3), 0, True, 2.0),
    (24, 1, 11, (1,), 12, False, None),
]


@pytest.mark.parametrize("task", ["classification", "regression"])
@pytest.mark.parametrize("act", MC.ACTS)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"FD{s[0]}Dn{s[1]}B{s[2]}NL{len(s[3])}D{s[4]}")
def test_stages_composed_equal_autograd(shape, act, task):
    FD, Dn, B, hidden, D, lin, cx = shape
    p = MC.make_mlp_inputs(FD, Dn, B, hidden, seed=1)
    gen = torch.Generator().manual_seed(B)
    y = (torch.rand(B, generator=gen) < 0.4).long() if task == "classification" else torch.randn(B, generator=gen)
    kw = dict(D=D, grad_scale=0.25 if B % 2 else 1.0)
    if lin:
        kw.update(lin_w=torch.randn(Dn, generator=gen), lin_w0=torch.randn(1, generator=gen))
    if cx is not None:
        kw.update(extra=torch.randn(B, generator=gen), coef_extra=cx)
    got = _compose(p, act, y, task, **kw)
    want = M.mlp_autograd_ref(p["xe"], p["xd"], p["Ws"], p["bs"], p["w_out"], p["w0"], act, y, task, **kw)
    for k in ("dnn", "z", "pred", "loss", "g", "xe", "w_out", "w0"):
        _rel(got[k], want[k].reshape(got[k].shape), k)
    for l in range(len(hidden)):
        _rel(got["h"][l], want["h"][l], f"h{l}")
        _rel(got["W"][l], want["W"][l], f"dW{l}")
        _rel(got["b"][l], want["b"][l], f"db{l}")
    if lin:
        _rel(got["lin_w"], want["lin_w"], "d_xd_wsum")
        _rel(got["lin_w0"], want["lin_w0"], "d_g_sum")


def test_clip_region_passes_no_gradient_in_both_references():
    p = MC.make_mlp_inputs(8, 0, 6, (4,), seed=2)
    y = torch.tensor([0, 1, 0, 1, 0, 1])
    extra = torch.tensor([25.0, 25.0, -25.0, -25.0, 30.0, -30.0])
    got = _compose(p, "relu", y, "classification", extra=extra)
    want = M.mlp_autograd_ref(p["xe"], None, p["Ws"], p["bs"], p["w_out"], p["w0"], "relu", y, "classification",
                              extra=extra)
    assert float(got["z"].abs().min()) > 17
    assert torch.equal(got["g"], torch.zeros(6, dtype=F64)) and torch.equal(want["g"], torch.zeros(6, dtype=F64))
    _rel(got["loss"], want["loss"], "loss in the clip region")


def test_dnn_stages_equal_the_oracle_layers():
    spec, p, idx, dense, y, hp = make_case("deepfm", B=23, F=4, D=8, Dn=3, hidden=(16, 8), dtype=F64)
    E, _ = T.feat_embedding_layer(p, spec, idx)
    want = T.dnn(p, T.dnn_input(E, dense), 2, activation="relu").reshape(-1)
    h = E.reshape(23, -1)
    h = torch.cat([h, dense], 1)
    for l in range(2):
        h, _ = M.layer_ref(h, p[f"dnn_layer_{l}_weights"], p[f"dnn_layer_{l}_bias"], "relu")
    got, _ = M.logit_ref(h, p["dnn_w"].reshape(-1), p["dnn_w0"])
    _rel(got, want, "dnn logit")


# ------------------------------------------------------------------------------------- fp32 emulation vs the bounds
def _emulate(p, act, D):
    """Every stage in torch fp32 on the CPU from fp32 inputs, each held to the bound the GPU module uses for it, with
    the float64 reference taken from the emulation's own fp32 intermediates (the GPU module's method)."""
    xe, xd, Ws, bs, w_out, w0, g = (p[k] for k in ("xe", "xd", "Ws", "bs", "w_out", "w0", "g"))
    x = xe if xd is None else torch.cat([xe, xd], 1)
    NL, B, FD = len(Ws), xe.shape[0], xe.shape[1]
    act32 = lambda v: R.bias_act_ref32(v, None, act)
    h = []
    for l in range(NL):
        hp = x if l == 0 else h[l - 1]
        h.append(act32(hp @ Ws[l] + bs[l]))
        ref, ab = M.layer_ref(hp, Ws[l], bs[l], act)
        R.assert_within(h[l], ref, R.sum_bound(Ws[l].shape[0] + 1, ab), f"h{l}")            # n = K_l + 1
    ref, ab = M.logit_ref(h[-1], w_out, w0)
    R.assert_within(h[-1] @ w_out + w0, ref, R.sum_bound(w_out.shape[0] + 1, ab), "logit")   # n = H + 1
    dh = [None] * NL
    dh[-1] = g[:, None] * w_out[None, :] * R._slope(h[-1], act)
    ref, ab = M.dh_last_ref(g, w_out, h[-1], act)
    R.assert_within(dh[-1], ref, R.sum_bound(w_out.shape[0] + 1, ab), "dh_last")             # n = H + 1
    for l in range(NL - 1, 0, -1):
        dh[l - 1] = (dh[l] @ Ws[l].T) * R._slope(h[l - 1], act)
        ref, ab = M.dh_prev_ref(dh[l], Ws[l], h[l - 1], act)
        R.assert_within(dh[l - 1], ref, R.sum_bound(Ws[l].shape[1] + 1, ab), f"dh{l - 1}")   # n = H_l + 1
    H0 = Ws[0].shape[1]
    d_rows = dh[0] @ Ws[0][:FD].T
    S = None
    if D:
        S = MC.fm_sum32(xe, D)
        d_rows = d_rows + g[:, None] * (S.repeat(1, FD // D) - xe)
    ref, ab = M.d_rows_ref(dh[0], Ws[0], FD, g, S, xe if D else None)
    R.assert_within(d_rows, ref, R.sum_bound(H0 + 2, ab), "d_rows")                          # n = H0 + 2
    ref, ab = M.dW0_ref(x, dh[0])
    R.assert_within(x.T @ dh[0], ref, R.sum_bound(B, ab), "dW0")                             # n = B
    for l in range(1, NL):
        ref, ab = M.dW_ref(h[l - 1], dh[l])
        R.assert_within(h[l - 1].T @ dh[l], ref, R.sum_bound(B, ab), f"dW{l}")               # n = B
    for l in range(NL):
        ref, ab = M.db_ref(dh[l])
        R.assert_within(dh[l].sum(0), ref, R.sum_bound(B, ab), f"db{l}")                     # n = B
    ref, ab = M.d_w_out_ref(h[-1], g)
    R.assert_within(h[-1].T @ g, ref, R.sum_bound(B, ab), "d_w_out")                         # n = B
    ref, ab = M.sum_g_ref(g)
    R.assert_within(g.sum().reshape(1), ref, R.sum_bound(B, ab), "sum g")                    # n = B
    if xd is not None:
        ref, ab = M.d_xd_wsum_ref(xd, g)
        R.assert_within(g @ xd, ref, R.sum_bound(B, ab), "d_xd_wsum")                        # n = B


FM_D = {64: 16, 60: 4, 96: 12, 320: 32, 192: 64, 448: 64, 256: 64, 416: 32}  # an FM width that divides FD, where any


@pytest.mark.parametrize("case", MC.loader_cases() + list(MC.GRID_STRIDE_CASES),
                         ids=lambda c: f"FD{c[0]}Dn{c[1]}B{c[2]}H{'x'.join(map(str, c[3]))}{c[4]}")
def test_fp32_emulation_stays_inside_the_bounds_at_the_gpu_shapes(case):
    FD, Dn, B, hidden, act = case
    p = MC.make_mlp_inputs(FD, Dn, B, hidden)
    _emulate(p, act, FM_D.get(FD, 0))


def test_head_restatement_in_fp32_meets_the_tolerances():
    """The head in torch fp32 against head_ref: logit inside the branch-sum bound (n = 3), pred / dlogit / loss at the
    transcendental tolerance, the loss and gradient taken from the fp32 probabilities."""
    B = 257
    gen = torch.Generator().manual_seed(3)
    dnn, a, b = (torch.randn(B, generator=gen) * 2 for _ in range(3))
    y = (torch.rand(B, generator=gen) < 0.4).long()
    ca, cb, cm = 2.0, -0.5, 1.0
    z32 = ca * a + cb * b + cm * dnn
    p32 = torch.sigmoid(z32)
    head = M.head_ref(dnn, [(a, ca), (b, cb)], cm, y, "classification", 0.25)
    R.assert_within(z32, head["logit"], R.sum_bound(3, head["logit_abs"]), "logit")
    R.close(p32, head["pred"], what="pred")
    head = M.head_ref(dnn, [(a, ca), (b, cb)], cm, y, "classification", 0.25, pred=p32)
    pc = p32.clamp(1e-7, 1 - 1e-7)
    t = y.float()
    dz32 = -(t / (pc + 1e-7) - (1 - t) / (1 - pc + 1e-7)) * p32 * (1 - p32)
    R.close(dz32 / B * 0.25, head["dlogit"], what="dlogit")
    R.close(-(t * torch.log(pc + 1e-7) + (1 - t) * torch.log(1 - pc + 1e-7)).mean().reshape(1), head["loss"], what="loss")


def test_mlp_tail_wrapper_refuses_a_scaled_mlp_logit():
    """dlogit = dLoss/d(final logit) is the MLP's own output gradient only for coef_mlp = 1 (include/recman_hip.h)."""
    from recman_amd import ops

    for coef in (2.0, -0.5):
        with pytest.raises(ValueError, match="coef_mlp must be 1"):
            ops.mlp_tail(4, [], coef, y=torch.zeros(4, dtype=torch.int64), dlogit=None, loss_partial=None, dh=[])
