"""Hyper-parameter dictionaries with the reference's keys and defaults
(recman/tf/hparams/xDeepFM.py:7-34, BaseHyperParameters.py:67-100), minus TensorBoard:
`HParam(domain)` keeps a plain list of candidate values and grid_search() yields dicts."""
import itertools


class HParam:
    def __init__(self, name, default_value):
        assert name
        self.name = name
        self.default_value = default_value
        self.hp_domain = [default_value]

    def __call__(self, domain=None):
        self.hp_domain = list(domain) if domain is not None else [self.default_value]
        return self


class BaseHyperParameters(dict):
    LearningRate = "learning_rate"
    Optimizer = "optimizer"

    # the wide part (the table's bias and linear entries, linear_w_dense) may train by a rule of its own - the
    # Wide&Deep recipe: FTRL with L1 there, Adam / Adagrad on the embeddings and the DNN (not in the reference)
    LinearOptimizer = "linear_optimizer"        # None: the same as `optimizer`; adam | adagrad | sgd | gd | ftrl
    LinearLearningRate = "linear_learning_rate"  # None: `learning_rate`
    FtrlL1 = "ftrl_l1"
    FtrlL2 = "ftrl_l2"
    FtrlBeta = "ftrl_beta"

    # a ranking objective next to the log loss (not in the reference; include/recman_hip_rank.h): the single-logit
    # models minimise (1 - rank_loss_weight) log loss + rank_loss_weight L, L over the examples of ONE batch that share
    # an id of the feature rank_group_by.  Gen-2 classes read the keys from their hparams dict, gen-1 classes from
    # model.hparams
    RankLoss = "rank_loss"              # None | "pairwise" (RankNet / BPR pairs) | "listwise" (ListNet softmax)
    RankGroupBy = "rank_group_by"       # the name of a SparseFeat, or None: the whole batch is one list
    RankLossWeight = "rank_loss_weight"  # alpha, 0 < alpha <= 1
    RankNorm = "rank_norm"              # "group": every scored group weighs its impressions | "pairs": every pair 1/Q

    def __init__(self):
        dict.__init__(self)
        self.add_param(self.LearningRate, 0.001)
        self.add_param(self.Optimizer, "adam")  # adam | adagrad | sgd | gd | momentum | ftrl
        self.add_param(self.LinearOptimizer, None)
        self.add_param(self.LinearLearningRate, None)
        self.add_param(self.FtrlL1, 0.0)
        self.add_param(self.FtrlL2, 0.0)
        self.add_param(self.FtrlBeta, 0.0)
        self.add_param(self.RankLoss, None)
        self.add_param(self.RankGroupBy, None)
        self.add_param(self.RankLossWeight, 0.5)
        self.add_param(self.RankNorm, "group")

    def add_param(self, name, default_val):
        self[name] = HParam(name, default_val)()

    def grid_search(self, print_hp=False):
        names = list(self.keys())
        for combo in itertools.product(*[self[n].hp_domain for n in names]):
            bag = dict(zip(names, combo))
            if print_hp:
                print(bag)
            yield bag

    def defaults(self):
        return {k: v.default_value for k, v in self.items()}


class xDeepFM(BaseHyperParameters):
    EmbeddingSize = "embedding_size"
    EmbeddingL2Reg = "embedding_l2_reg"
    LinearL2Reg = "linear_l2_reg"
    LinearFeatures = "linear_features"
    DeepHiddenUnits = "deep_hidden_units"
    DeepDropOut = "deep_dropout"
    DeepActivation = "deep_activation"
    DeepL2Reg = "deep_l2_reg"
    CinCrossLayerUnits = "cin_cross_layer_units"
    CinDropOut = "cin_dropout"
    CinActivation = "cin_activation"
    CinL2Reg = "cin_l2_reg"

    def __init__(self):
        BaseHyperParameters.__init__(self)
        self.add_param(self.EmbeddingSize, 8)
        self.add_param(self.EmbeddingL2Reg, 0.00001)
        self.add_param(self.LinearL2Reg, 0.00001)
        self.add_param(self.LinearFeatures, [])
        self.add_param(self.DeepHiddenUnits, (32, 32))
        self.add_param(self.DeepDropOut, (0.8, 0.8, 0.8))
        self.add_param(self.DeepActivation, "leaky_relu")
        self.add_param(self.DeepL2Reg, 0.00001)
        self.add_param(self.CinCrossLayerUnits, [100, 100, 100])
        self.add_param(self.CinDropOut, [1, 1, 1, 1])
        self.add_param(self.CinActivation, "leaky_relu")
        self.add_param(self.CinL2Reg, 0.00001)
