"""GPU: what InteractionEngine owns for DLRM, FiBiNET and PNN - the X / dX buffers with their pad columns, and the
flow E -> interaction -> DNN -> interaction backward - at the smallest shapes that still have a pad (hidden (8,)):
    DLRM     F=2, D=16, Dn=2             W = 19,  ldx = 20
    PNN      F=7, D=16, inner only       W = 133, ldx = 136;  the same with outer "vec"
    FiBiNET  F=3, D=8, "each"            W = ldx = 48: no pad
One engine runs batches of 130, then 5, then 130 rows.  After every forward and every fwd_bwd the columns W: of X and dX
are +0.0 as int32 words (the buffers are zero-filled once per batch size; nothing may write there, not even -0.0).  At
the last call loss, every entry of grads and d_rows meet the float64 twin under the helper and the bounds of the
model's own test_gpu_*_model.py (imported, not restated); d_rows against the gradient of the twin's gathered rows."""
import pytest
import torch

from oracle import th_layers as TL
from tests import dlrm_ref, fibinet_ref, pnn_ref
from tests import test_gpu_dlrm_model as dlrm_t
from tests import test_gpu_fibinet_model as fibinet_t
from tests import test_gpu_pnn_model as pnn_t
from tests.test_gpu_parity import _close_grad

pytestmark = pytest.mark.gpu
F32 = torch.float32
BATCHES = (130, 5, 130)

# model -> (its float64 restatement, its make_case call, the engine and the comparison of its own model test, W, ldx)
CASES = {
    "dlrm": (dlrm_ref, lambda lin: dlrm_ref.make_case(130, 2, 16, 2, hidden=(8,), use_linear=lin),
             lambda k: dlrm_t._engine(k["spec"], k["hp"], k["p"]), dlrm_t._compare, 19, 20),
    "pnn_inner": (pnn_ref, lambda lin: pnn_ref.make_case(pnn_ref.INNER, "mat", lin, (8,), 130, 7, 16, 3),
                  pnn_t._engine, pnn_t._compare, 133, 136),
    "pnn_outer_vec": (pnn_ref, lambda lin: pnn_ref.make_case(pnn_ref.OUTER, "vec", lin, (8,), 130, 7, 16, 3),
                      pnn_t._engine, pnn_t._compare, 133, 136),
    "fibinet_each": (fibinet_ref, lambda lin: fibinet_ref.make_case(130, 3, 8, 2, 3, "each", hidden=(8,),
                                                                    use_linear=lin),
                     fibinet_t._engine, fibinet_t._compare, 48, 48),
}
_TWINS = {}


def _twin(name, use_linear):
    """(case, the restatement's fwd_bwd over it, dLoss/dE [B,F,D] in float64), made once: the rows the restatement
    gathers keep their gradient."""
    key = (name, use_linear)
    if key not in _TWINS:
        R, make = CASES[name][:2]
        k = make(use_linear)
        assert k.get("min_abs_pre", k.get("model_min_abs_pre")) >= R.KINK
        gathered, real = [], TL.feat_embedding_layer

        def keeping(*a, **kw):
            E, bias = real(*a, **kw)
            E.retain_grad()
            gathered.append(E)
            return E, bias

        TL.feat_embedding_layer = keeping
        try:
            ref = R.fwd_bwd(*(k[n] for n in ("p", "spec", "idx", "dense", "y", "hp")))
        finally:
            TL.feat_embedding_layer = real
        assert len(gathered) == 1
        _TWINS[key] = (k, ref, gathered[0].grad)
    return _TWINS[key]


def _pads_are_plus_zero(e, when):
    torch.cuda.synchronize()
    for what, buf in (("X", e.X), ("dX", e.dX)):
        assert buf.shape == (e._B, e.ldx)
        words = buf[:, e.W:].contiguous().view(torch.int32)
        assert int(words.ne(0).sum()) == 0, f"{when}: {what}[:, {e.W}:] holds a word that is not +0.0"


@pytest.mark.parametrize("use_linear", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pad_columns_and_the_float64_twin_across_batch_sizes(hip_lib, name, use_linear):
    _, _, engine, compare, W, ldx = CASES[name]
    k, ref, d_rows64 = _twin(name, use_linear)
    e = engine(k)
    assert (e.W, e.ldx) == (W, ldx) and e.use_linear == use_linear and e.mlp.hidden == [8]
    idx, dense, y = k["idx"].cuda(), k["dense"].to(F32).cuda(), k["y"].cuda()
    for call, B in enumerate(BATCHES):
        rows = slice(0, B)
        e.forward(idx[rows].contiguous(), dense[rows].contiguous(), training=False)
        _pads_are_plus_zero(e, f"{name} forward {call} (B={B})")
        loss = e.fwd_bwd(idx[rows].contiguous(), dense[rows].contiguous(), y[rows].contiguous())
        _pads_are_plus_zero(e, f"{name} fwd_bwd {call} (B={B})")
    what = f"{name} linear={use_linear}: "
    compare(e, idx, loss, ref, what=what)
    print(f"{what}d_rows measure {CASES[name][0].grad_measure(e.d_rows, d_rows64):.2e}")
    _close_grad(e.d_rows, d_rows64, what=what + "d_rows")
