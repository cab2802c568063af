"""Host: what every front end of recman_amd.th owes sklearn and the engines, checked at construction (no GPU, no
engine): get_params() hands every constructor argument back as given, clone() rebuilds the same model, deep_dropout
reaches hparams as one keep probability per DNN input and hidden layer, loss_type picks the task, and the TF-only
arguments are stored.  One row of CASES per DeepModel subclass exported by recman_amd.th:
    kw      the arguments the class cannot do without, and a few non-default ones
    hidden  the argument that holds the DNN's hidden units (None: the model has no deep_dropout)
    none    deep_dropout=None is accepted and a wrong length is refused with "keep probabilities" at construction
    lists   list-valued hidden units come back from get_params() as the list given (the class stores them as given)
    clones  sklearn's clone() applies (xDeepFM keeps the reference's hyper-parameter-dict constructor and merges the
            defaults into the dict it stores, so clone()'s identity check cannot hold for it)
    loss    the class has loss_type (xDeepFM takes task itself; MMoE's tasks and TwoTower's loss are their own)"""
import inspect

import pytest
from sklearn.base import clone

from recman_amd import th

TF_KNOBS = dict(what_means_greater="auc", use_interactive_session=False, log_dir="./elsewhere")


def _fd():
    fd = th.FeatureDictionary()
    fd["u"] = th.SparseFeat("u", 5)
    fd["i"] = th.SparseFeat("i", 7)
    fd["x"] = th.DenseFeat("x")
    return fd


def _case(kw=None, hidden="deep_hidden_units", none=False, lists=False, clones=True, loss=True):
    return dict(kw=kw or {}, hidden=hidden, none=none, lists=lists, clones=clones, loss=loss)


FIXED = dict(deep_dropout=(0.9, 0.8, 0.7), deep_hidden_units=(16, 8))  # classes that store the tuples they build
CASES = {
    "AFM": _case(dict(att_factor=4, use_deep=False, l2_reg=0.2), hidden=None),
    "AutoInt": _case(dict(att_layer_num=2, deep_hidden_units=(16, 8)), none=True),
    "BST": _case(dict(FIXED, att_head_num=4, l2_reg=0.2)),
    "DCN": _case(dict(FIXED, cross_type="mix", cross_experts=2)),
    "DIEN": _case(dict(FIXED, l2_reg=0.2)),
    "DIN": _case(dict(FIXED, att_hidden_units=(8, 4), l2_reg=0.2)),
    "DLRM": _case(dict(bottom_hidden_units=[16, 8], deep_hidden_units=[16, 8]), none=True, lists=True),
    "DeepFM": _case(dict(FIXED, use_fm=False)),
    "FiBiNET": _case(dict(bilinear_type="all", deep_hidden_units=[16, 8]), none=True, lists=True),
    "FmFM": _case(dict(field_interaction="vector", deep_hidden_units=[16, 8]), none=True, lists=True),
    "FwFM": _case(dict(deep_hidden_units=[16, 8]), none=True, lists=True),
    "MaskNet": _case(dict(block_order="serial", num_blocks=2, block_hidden_units=16, deep_hidden_units=[16, 8]),
                     none=True, lists=True),
    "MMoE": _case(dict(task_names=("a", "b", "c"), task_types=("classification", "regression", "classification"),
                       expert_hidden_units=[16, 8], tower_hidden_units=[8]), hidden=None, lists=True, loss=False),
    "PNN": _case(dict(use_outer=True, kernel_type="vec", deep_hidden_units=[16, 8]), none=True, lists=True),
    "TwoTower": _case(dict(user_features=("u", "x"), item_features=("i",), item_id_feature="i",
                           user_hidden_units=[16, 8], item_hidden_units=[8]), hidden=None, lists=True, loss=False),
    "xDeepFM": _case(dict(hparams=dict(deep_hidden_units=(16, 8), deep_dropout=(0.9, 0.8, 0.7)), task="regression"),
                     clones=False, loss=False),
}


def _exported():
    return sorted(n for n in th.__all__ if inspect.isclass(getattr(th, n)) and issubclass(getattr(th, n), th.DeepModel)
                  and getattr(th, n) is not th.DeepModel)


def test_every_front_end_has_a_case():
    assert _exported() == sorted(CASES)


def _make(name, **more):
    c = CASES[name]
    kw = dict(c["kw"], **more)
    if "what_means_greater" in inspect.signature(getattr(th, name).__init__).parameters:
        kw = dict(TF_KNOBS, **kw)
    return getattr(th, name)(_fd(), **kw), kw


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructor_contract(name):
    c = CASES[name]
    m, kw = _make(name)
    assert m._engine is None
    # get_params(): every constructor argument, the given ones as given (the same object), the others at their default
    sig = inspect.signature(type(m).__init__).parameters
    params = m.get_params(deep=False)
    assert set(params) == set(sig) - {"self"}
    for k, v in params.items():
        if k == "hparams":  # xDeepFM: the given keys over the defaults
            assert all(v[a] == b for a, b in kw[k].items()) and set(v) == set(th.hparams.xDeepFM().defaults())
        elif k in kw:
            assert v is kw[k], (k, v, kw[k])
        elif k != "feat_dict" and c["clones"]:
            assert v == sig[k].default, (k, v, sig[k].default)
    if c["lists"]:
        assert any(isinstance(v, list) for v in kw.values())
    # clone(): the same class, no engine, the same hyper-parameters
    if c["clones"]:
        twin = clone(m)
        assert type(twin) is type(m) and twin._engine is None and twin.hparams == m.hparams
        assert list(twin.hparams) == list(m.hparams)
    # the three TF-only knobs are stored
    for k, v in TF_KNOBS.items():
        if k in sig:
            assert getattr(m, k) == v
    # deep_dropout: one keep probability for the DNN's input and for every hidden layer
    if c["hidden"] is not None:
        hidden = m.hparams[c["hidden"]]
        assert len(m.hparams["deep_dropout"]) == len(hidden) + 1
    if c["loss"]:
        assert m.task == "classification" and m.loss_type == "logloss"
        r, _ = _make(name, loss_type="mse")
        assert r.task == "regression" and r.loss_type == "mse"
    elif name == "xDeepFM":
        assert m.task == "regression"


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["none"]))
def test_deep_dropout_none_and_wrong_length(name):
    c = CASES[name]
    m, kw = _make(name, deep_dropout=None)
    hidden = m.hparams[c["hidden"]]
    assert m.get_params()["deep_dropout"] is None and clone(m).deep_dropout is None
    assert tuple(m.hparams["deep_dropout"]) == (1,) * (len(hidden) + 1)
    given = [0.9] * (len(hidden) + 1)
    m, _ = _make(name, deep_dropout=given)
    assert m.get_params()["deep_dropout"] is given and tuple(m.hparams["deep_dropout"]) == tuple(given)
    for bad in ([0.9] * len(hidden), [0.9] * (len(hidden) + 2)):
        with pytest.raises(ValueError, match="keep probabilities"):
            _make(name, deep_dropout=bad)
