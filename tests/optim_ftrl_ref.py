"""CPU PyTorch restatement (dtype-generic) of FTRL-Proximal and of the two-rule row-wise step of csrc/optim.hip, on
the cases of tests/optim_ref.py.

TEST INFRASTRUCTURE.  A row-wise step carries an EMBEDDING rule (columns 0 .. D-1 of a row, state in the [R, 2 D]
moment array) and a SIDE rule (columns D, D + 1: bias and linear entry, state in the row's columns D+2 .. D+5).  Each
is Adam, Adagrad or SGD as optim_ref.update states them, or FTRL (tf.keras.optimizers.Ftrl, learning_rate_power -0.5,
initial accumulator 0.1, no l2_shrinkage), per element and in exactly this order of operations:

    n_new = n + g*g
    sigma = (sqrt(n_new) - sqrt(n)) / lr
    z     = z + g - sigma * p
    q     = (sqrt(n_new) + beta) / lr + 2*l2
    p     = |z| > l1 ? (copysign(l1, z) - z) / q : 0
    n     = n_new

g is the summed gradient of the row after the lazy l2 term; `reset` sets z = 0, n = 0.1 first.  z lives in the m slot
and n in the v slot.  reference(case, torch.float32) rounds after every operation, as the kernel does (it compiles
the FTRL branch without contraction into fused multiply-adds), and is the yardstick of optim_ref.compare's bounds;
`mutate` restates the step deliberately wrong (tests/test_optim_ftrl_host.py: the bounds catch each mutation).

Every hyper-parameter crosses the C ABI as a float: the restatement computes with the float32-rounded values.
"""
import torch

from tests import optim_ref as R

RULES = ("adam", "adagrad", "sgd", "ftrl")
MUTATIONS = ("side_reads_emb_n", "swap_z_n", "l2_once", "l1_on_p", "side_rule_on_emb")
F32, F64 = torch.float32, torch.float64


def has_m(rule):
    return rule in ("adam", "ftrl")


def has_v(rule):
    return rule != "sgd"


# -------------------------------------------------------------------------------------------------------- the rule
def ftrl_update(p, z, n, g, lr, l1, l2, beta, reset, mutate=None):
    """FTRL on whole arrays of one dtype: new (p, z, n).  Every line is one rounding in float32."""
    if mutate == "swap_z_n":   # the kernel reading z where n lives and n where z lives (and writing them back so)
        z, n = n, z
    if reset:
        z, n = torch.zeros_like(z), torch.full_like(n, R.f32(0.1))
    gg = g * g
    n_new = n + gg
    root_new, root = n_new.sqrt(), n.sqrt()
    sigma = (root_new - root) / lr
    sp = sigma * p
    z = z + g
    z = z - sp
    q = (root_new + beta) / lr
    q = q + (l2 if mutate == "l2_once" else 2.0 * l2)
    over = (p.abs() if mutate == "l1_on_p" else z.abs()) > l1
    shrunk = (torch.copysign(torch.full_like(z, l1), z) - z) / q
    p = torch.where(over, shrunk, torch.zeros_like(p))
    if mutate == "swap_z_n":
        return p, n_new, z
    return p, z, n_new


def rule_update(rule, p, m, v, G, dtype, case, lr, t, reset, mutate=None):
    """One rule on whole arrays: new (p, m, v); slots the rule does not keep come back unchanged."""
    if rule == "ftrl":
        return ftrl_update(p, m, v, G, R.f32(lr), R.f32(case["l1"]), R.f32(case["ftrl_l2"]), R.f32(case["ftrl_beta"]),
                           reset, mutate)
    return R.update(rule, p, m, v, G, dtype, R.f32(lr), R.lr_t_of(dict(case, lr=lr), t), R.f32(case["beta1"]),
                    R.f32(case["beta2"]), R.f32(case["eps"]), reset)


def tf_apply_ftrl(var, accum, linear, grad, lr, l1, l2, beta, lr_power=-0.5):
    """A second, independent statement: the arithmetic of TensorFlow's ApplyFtrl (training_ops.cc, FtrlCompute without
    l2_shrinkage) as Keras's Ftrl calls it - beta folded into l2 as l2 + beta / (2 lr), powers instead of square
    roots, the soft threshold as a clip - composed of torch ops.  Returns (var, accum, linear)."""
    l2_adjusted = l2 + beta / (2.0 * lr)
    new_accum = torch.addcmul(accum, grad, grad)
    sigma = (torch.pow(new_accum, -lr_power) - torch.pow(accum, -lr_power)) / lr
    linear = linear + grad - sigma * var
    quadratic = torch.pow(new_accum, -lr_power) / lr + 2.0 * l2_adjusted
    var = (torch.clamp(linear, -l1, l1) - linear) / quadratic
    return var, new_accum, linear


# ---------------------------------------------------------------------------------------------------- the cases
def state_of(rows, mom, D, emb, side):
    """Kernel layout -> (p, m, v), each [R, D + 2] float64 on the CPU; a slot its part's rule does not keep reads 0."""
    rows = rows.detach().cpu().double()
    p = rows[:, : D + 2].clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    if has_v(emb):
        me, ve = R.deinterleave(mom.detach().cpu().double(), D)
        v[:, :D] = ve
        if has_m(emb):
            m[:, :D] = me
    if has_v(side):
        v[:, D:] = rows[:, D + 4: D + 6]
        if has_m(side):
            m[:, D:] = rows[:, D + 2: D + 4]
    return p, m, v


def reseed(case, emb, side=None, side_lr=None, l1=0.0, ftrl_l2=0.0, ftrl_beta=0.0):
    """An optim_ref case (built for "adam": the occurrences, gradients and parameters depend on neither kind nor
    rule) with the state of the two rules: zeros, Adagrad's and FTRL's accumulator at 0.1, and SENTINEL wherever a
    rule keeps nothing - the m halves under an Adagrad embedding rule, m_b m_l under an Adagrad side rule, all four
    state columns under an SGD side rule; no moment array under an SGD embedding rule."""
    assert case["kind"] == "adam"
    side = emb if side is None else side
    assert emb in RULES and side in RULES
    D, Rn = case["D"], case["R"]
    c = dict(case, kind=emb, side=side, side_lr=case["lr"] if side_lr is None else side_lr, l1=l1, ftrl_l2=ftrl_l2,
             ftrl_beta=ftrl_beta)
    rows0 = case["rows0"].clone()
    rows0[:, D + 2: D + 6] = R.SENTINEL
    if has_v(side):
        rows0[:, D + 4: D + 6] = 0.1 if side in ("adagrad", "ftrl") else 0.0
    if has_m(side):
        rows0[:, D + 2: D + 4] = 0.0
    c["rows0"] = rows0
    c["mom0"] = None
    if has_v(emb):
        m0 = torch.zeros(Rn, D) if has_m(emb) else torch.full((Rn, D), R.SENTINEL)
        c["mom0"] = R.interleave(m0, torch.full((Rn, D), 0.1 if emb in ("adagrad", "ftrl") else 0.0))
    return c


def ftrl_columns(case):
    """Boolean [D + 2]: the columns FTRL updates."""
    D = case["D"]
    cols = torch.zeros(D + 2, dtype=torch.bool)
    cols[:D] = case["kind"] == "ftrl"
    cols[D:] = case["side"] == "ftrl"
    return cols


def median_l1(case):
    """About the median |z| of the touched FTRL elements after step 1, from the float64 reference (z after the first
    step does not depend on l1): with it the soft threshold cuts through the middle of the case's elements."""
    ref = reference(dict(case, l1=0.0), F64, steps=1)
    rows = R.occurrence_rows(case, 0)
    touched = torch.zeros(case["R"], dtype=torch.bool)
    touched[rows[rows >= 0]] = True
    z = ref[0][1][touched][:, ftrl_columns(case)].abs().reshape(-1)
    return R.f32(float(z[z > 0].median()))   # (z = 0: an entry without a gradient, g_lin / g_bias absent)


def make_case(D, kind, entry, side=None, side_lr=None, l1="median", ftrl_l2=0.0, ftrl_beta=0.0, **opts):
    """optim_ref.make_case with two rules (side None: one rule) and FTRL's constants; l1 "median": median_l1."""
    c = reseed(R.make_case(D, "adam", entry, **opts), kind, side, side_lr, 0.0, ftrl_l2, ftrl_beta)
    if "ftrl" in (c["kind"], c["side"]):
        c["l1"] = median_l1(c) if l1 == "median" else l1
    return c


def threshold_shares(case, want):
    """[(share of the touched FTRL elements with |z| > l1, with |z| <= l1)] after every step of the float64
    reference `want` - touched: by this step or an earlier one."""
    cols, seen, out = ftrl_columns(case), torch.zeros(case["R"], dtype=torch.bool), []
    for s in range(len(case["steps"])):
        rows = R.occurrence_rows(case, s)
        seen[rows[rows >= 0]] = True
        z = want[s][1][seen][:, cols].abs().reshape(-1)
        over = float((z > case["l1"]).double().mean())
        out.append((over, 1.0 - over))
    return out


# -------------------------------------------------------------------------------------------------- the restatement
def reference(case, dtype=F64, mutate=None, steps=None):
    """[(p, m, v) after step s], each [R, D + 2] float64: columns < D by the embedding rule, columns D, D + 1 by the
    side rule.  Slots a rule does not keep stay 0."""
    D, emb, side = case["D"], case["kind"], case["side"]
    p, m, v = (x.to(dtype) for x in state_of(case["rows0"], case["mom0"], D, emb, side))
    l2e, l2l = R.f32(case["l2_emb"]), R.f32(case["l2_lin"])
    out = []
    for s in range(len(case["steps"]) if steps is None else steps):
        G, touched = R.run_sums(case, s, dtype)
        G = G.clone()
        G[:, :D] += l2e * p[:, :D]
        G[:, D + 1] += l2l * p[:, D + 1]
        reset = s in case["reset_at"]
        t = 1 if reset else case["step0"] + s
        v_in = v
        if mutate == "side_reads_emb_n":   # the side entries read the n (v) of the last embedding slice
            v_in = v.clone()
            v_in[:, D: D + 2] = v[:, D - 4: D - 2]
        by_side = rule_update(side, p, m, v_in, G, dtype, case, case["side_lr"], t, reset, mutate)
        by_emb = by_side if mutate == "side_rule_on_emb" else rule_update(emb, p, m, v_in, G, dtype, case, case["lr"],
                                                                         t, reset, mutate)
        new = [torch.cat([a[:, :D], b[:, D:]], dim=1) for a, b in zip(by_emb, by_side)]
        tm = touched[:, None]
        p, m, v = torch.where(tm, new[0], p), torch.where(tm, new[1], m), torch.where(tm, new[2], v)
        out.append((p.double(), m.double(), v.double()))
    return out


def dense_reference(p0, grads, dtype=F64, lr=0.01, l1=0.0, l2=0.0, beta=0.0, reset_at=()):
    """rm_dense_optimizer_step_rule with kind 3 restated: [(p, z, n) after every step] as float64."""
    p = p0.to(dtype)
    z, n = torch.zeros_like(p), torch.full_like(p, R.f32(0.1))
    out = []
    for s, g in enumerate(grads):
        p, z, n = ftrl_update(p, z, n, g.to(dtype), R.f32(lr), R.f32(l1), R.f32(l2), R.f32(beta), s in reset_at)
        out.append((p.double(), z.double(), n.double()))
    return out


# ------------------------------------------------------------------------------------------------------ the bounds
def compare(got, want, ref32, case, tag="", show=True):
    """optim_ref.compare's bounds.  One rule: on the whole state, as tests/test_gpu_optim_kernels.py does.  Two rules:
    on the embedding columns and the side columns apart, each with the slots its own rule keeps (the bound of a part
    is then taken from that part's own values and restatement: never a wider one)."""
    D, emb, side = case["D"], case["kind"], case["side"]

    def pick(state, sl, rule):
        return (state[0][:, sl], state[1][:, sl] if has_m(rule) else None, state[2][:, sl] if has_v(rule) else None)

    if emb == side:
        sl = slice(None)
        return R.compare(pick(got, sl, emb), pick(want, sl, emb), pick(ref32, sl, emb), D, tag=tag, show=show)
    bad = []
    for part, sl, rule in (("emb", slice(0, D), emb), ("side", slice(D, D + 2), side)):
        bad += [(f"{part} {q[0]}",) + q[1:] for q in R.compare(pick(got, sl, rule), pick(want, sl, rule),
                                                              pick(ref32, sl, rule), None,
                                                              tag=f"{tag} {part}[{rule}]", show=show)]
    return bad


# ------------------------------------------------------------------------- the cases of the GPU file, by their names
FTRL_CASES = {f"d{D}_ftrl_{entry}": dict(D=D, kind="ftrl", entry=entry) for D in R.WIDTHS for entry in R.ENTRIES}
# (embedding rule, side rule); G = 4, 8, 32: the side lanes sit in different places of the lane group
SPLIT_PAIRS = (("adam", "ftrl"), ("adagrad", "ftrl"), ("sgd", "ftrl"), ("ftrl", "adam"), ("ftrl", "sgd"))
SPLIT_CASES = {f"d{D}_{emb}_{side}_{R.ENTRIES[i % 3]}": dict(D=D, kind=emb, side=side, entry=R.ENTRIES[i % 3])
               for D in (8, 24, 64) for i, (emb, side) in enumerate(SPLIT_PAIRS)}
OPTION_CASES = {}
for _D in (12, 64):
    _o = {
        "reset": dict(kind="ftrl", entry="fields", reset_at=(2,)),
        "reset_split": dict(kind="adagrad", side="ftrl", entry="rows", reset_at=(2,)),
        "l2_lazy": dict(kind="ftrl", entry="pairs", l2_emb=3e-2, l2_lin=2e-2),
        "lin_mask": dict(kind="adam", side="ftrl", entry="fields", lin_mask=(1.0, 0.0, 1.0), l2_lin=2e-2),
        "no_bias_no_lin": dict(kind="ftrl", entry="pairs", no_bias=True, no_lin=True),
        "no_lin": dict(kind="adagrad", side="ftrl", entry="fields", no_lin=True),
        "ld_d8": dict(kind="ftrl", entry="fields", ld=_D + 8),
        "ld_d12": dict(kind="adagrad", side="ftrl", entry="rows", ld=_D + 12),
        "l1_zero": dict(kind="ftrl", entry="rows", l1=0.0),
        "l2_beta": dict(kind="ftrl", entry="fields", ftrl_l2=0.5, ftrl_beta=1.0),
        "side_lr": dict(kind="ftrl", side="ftrl", entry="pairs", side_lr=0.05),
        "side_lr_adagrad": dict(kind="adagrad", side="adagrad", entry="fields", side_lr=0.05),
        "hyper": dict(kind="adam", side="ftrl", entry="rows", lr=0.037, side_lr=0.2, ftrl_beta=0.5),
    }
    for _k, _v in _o.items():
        OPTION_CASES[f"d{_D}_{_k}"] = dict(D=_D, **_v)
