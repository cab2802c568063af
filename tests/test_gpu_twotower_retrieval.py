"""GPU: retrieval through th.TwoTower - index_items, retrieve, evaluate_catalogue - on a small model (towers (16, 8),
one fit_on_batch step) over a catalogue of 300 items, one of them listed twice.  retrieve() is held to the float64
top-k of its own embeddings (user_embeddings @ item_embeddings^T / temperature) under the near-tie rule of
tests/test_gpu_topk.py; evaluate_catalogue() to a host recomputation from retrieve()."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import test_gpu_topk as TK
from tests import topk_ref as R

pytestmark = pytest.mark.gpu
N_ITEMS, N_USERS = 299, 37   # item ids 1..299; the catalogue repeats item 5 as its last row (300 rows)
TEMPERATURE = 0.05


def _item_cols(items):
    items = np.asarray(items, dtype=np.int64)
    return dict(item=items, icat=1 + items % 6, di=(((items * 37) % 17) / 17.0 - 0.5).astype(np.float32))


def _user_cols(g, n):
    return dict(u0=g.integers(1, 20, n), du=g.standard_normal(n).astype(np.float32))


def _fd():
    import recman_amd.th as th

    fd = th.FeatureDictionary()
    for n, V in (("u0", 19), ("item", N_ITEMS), ("icat", 6)):
        fd[n] = th.SparseFeat(n, V)
        fd[n].encoder.fit(np.arange(1, V + 1))
    fd["du"], fd["di"] = th.DenseFeat("du", scaler=False), th.DenseFeat("di", scaler=False)
    return fd


@pytest.fixture(scope="module")
def setup(hip_lib):
    import recman_amd.th as th

    torch.manual_seed(0)
    g = np.random.default_rng(5)
    m = th.TwoTower(_fd(), user_features=("u0", "du"), item_features=("item", "icat", "di"), item_id_feature="item",
                    user_hidden_units=(16, 8), item_hidden_units=(16, 8), embedding_size=8, temperature=TEMPERATURE,
                    batch_size=64, recall_at=(1, 5, 10), learning_rate=0.01)
    train = pd.DataFrame(dict(_user_cols(g, 64), **_item_cols(g.integers(1, N_ITEMS + 1, 64))))
    m.fit_on_batch(train)
    catalogue = pd.DataFrame(_item_cols(list(range(1, N_ITEMS + 1)) + [5]))
    users = pd.DataFrame(_user_cols(g, N_USERS))
    return m.index_items(catalogue), catalogue, users, train


def _case(m, catalogue, users, k):
    """The float64 top-k of the model's own float32 embeddings, as a tests/topk_ref random case."""
    ue, ie = m.user_embeddings(users), m.item_embeddings(catalogue)
    S = torch.from_numpy(ue).double() @ torch.from_numpy(ie).double().t() / TEMPERATURE
    rows, sc = R.topk(S, k + 1)
    kth, nxt = sc[:, k - 1], sc[:, k]
    tie = (kth - nxt).abs() <= R.TT.TIE * kth.abs().clamp(min=1.0)
    S32 = (torch.from_numpy(ue) @ torch.from_numpy(ie).t()) * np.float32(1.0 / TEMPERATURE)
    return dict(rows=rows[:, :k], scores=sc[:, :k], S=S, S32=S32, boundary_tie=tie, ie=ie)


def test_retrieve_matches_float64_and_excludes(setup):
    m, catalogue, users, _ = setup
    assert m._index["emb"].shape == (300, 8) and m._index["emb"].is_cuda
    assert list(m._index["item_id"][[4, 299]]) == [5, 5]
    case = _case(m, catalogue, users, 10)
    assert np.array_equal(case["ie"][4], case["ie"][299])  # the listed-twice item: one embedding, a tie by row
    rows, scores = m.retrieve(users, 10)
    assert rows.shape == (N_USERS, 10) and rows.dtype == np.int64 and scores.dtype == np.float32
    out = dict(rows=torch.from_numpy(rows), scores=torch.from_numpy(scores))
    TK._check_random(out, case, "TwoTower.retrieve")
    both = (rows == 4).any(1) & (rows == 299).any(1)
    for i in np.nonzero(both)[0]:
        assert list(rows[i]).index(4) < list(rows[i]).index(299)
    # exclude: each user's two best rows (with a duplicate and out-of-range rows) -> the next ten of a k = 12 call
    r12, s12 = m.retrieve(users, 12)
    ex = [[int(r[1]), -1, int(r[0]), 10 ** 6, int(r[1])] for r in r12]
    r10, s10 = m.retrieve(users, 10, exclude=ex)
    assert np.array_equal(r10, r12[:, 2:]) and np.array_equal(s10.view(np.int32), s12[:, 2:].view(np.int32))
    assert np.array_equal(r12[:, :10], rows) and np.array_equal(s12[:, :10].view(np.int32), scores.view(np.int32))


def test_evaluate_catalogue(setup):
    m, catalogue, users, _ = setup
    r, _ = m.retrieve(users, 10)
    ids = m._index["item_id"]
    # every third row's item is its top-1, the next row's its 8th: hits at different k
    own = np.array([ids[r[i, 0]] if i % 3 == 0 else ids[r[i, 7]] if i % 3 == 1 else 1 + (7 * i) % N_ITEMS
                    for i in range(N_USERS)])
    X = pd.DataFrame(dict(users, **_item_cols(own)))
    y = (np.arange(N_USERS) % 4 != 3).astype(np.float32)
    got = m.evaluate_catalogue(X, y)
    assert len(got) == 3 and m.catalogue_metric_names == ["catalogue_recall@1", "catalogue_recall@5",
                                                          "catalogue_recall@10"]
    # a host recomputation from retrieve(): a row is a hit at k if one of its top-k rows carries its own item id
    rows, _ = m.retrieve(X, 10)
    hit = ids[rows] == own[:, None]
    live = y > 0
    want = [float(hit[live, :k].any(1).sum()) / live.sum() for k in (1, 5, 10)]
    print(f"catalogue recall {got}, host {want}")
    assert got == want and 0.0 < got[0] <= got[1] < got[2] <= 1.0  # (no row's item is its 2nd..5th)
    # batch size and row order change nothing
    bs = m.batch_size
    try:
        m.batch_size = 7
        assert m.evaluate_catalogue(X, y) == got
    finally:
        m.batch_size = bs
    perm = np.random.default_rng(1).permutation(N_USERS)
    assert m.evaluate_catalogue(X.iloc[perm].reset_index(drop=True), y[perm]) == got
    assert m.evaluate_catalogue(X) == [float(hit[:, :k].any(1).sum()) / N_USERS for k in (1, 5, 10)]


def test_fit_and_restore_drop_the_index(setup, tmp_path):
    m, catalogue, users, train = setup
    path = str(tmp_path / "model")
    m.save(path)
    m.fit_on_batch(train)
    with pytest.raises(RuntimeError, match="index_items"):
        m.retrieve(users, 10)
    m.index_items(catalogue)
    assert m.retrieve(users, 3)[0].shape == (N_USERS, 3)
    m.restore(path)
    with pytest.raises(RuntimeError, match="index_items"):
        m.evaluate_catalogue(pd.DataFrame(dict(users, **_item_cols(np.ones(N_USERS, np.int64)))))
    m.index_items(catalogue)
