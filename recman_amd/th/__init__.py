"""The `recman.th`-shaped surface: the PyTorch backend the reference leaves as an empty
stub (recman/th/layers.py is 0 bytes, recman/th/DeepFM.py:12-13 is `pass`), here backed
by hand-written gfx950 kernels.  Same class names, constructor arguments and
fit()/predict()/evaluate() signatures as recman/tf/core."""
from .AFM import AFM
from .AutoInt import AutoInt
from .BestModelFinder import BestModelFinder
from .DCN import DCN
from .DLRM import DLRM
from .DeepFM import DeepFM
from .FiBiNET import FiBiNET
from .FmFM import FmFM, FwFM
from .MaskNet import MaskNet
from .MMoE import MMoE, PLE
from .PNN import PNN
from .TwoTower import TwoTower
from .BST import BST
from .DIEN import DIEN
from .DIN import DIN
from .DeepModel import DeepModel
from .inputs import (DataInputs, DenseFeat, FeatureDictionary, MultiValCsvFeat, ResilientLabelEncoder,
                     SequenceFeat, SparseFeat, SparseValueFeat)
from .xDeepFM import xDeepFM
from . import hparams
from . import layers

__all__ = ["AFM", "AutoInt", "BST", "BestModelFinder", "DCN", "DIEN", "DIN", "DLRM", "DeepFM", "DeepModel", "FiBiNET", "FmFM", "FwFM", "MaskNet", "MMoE", "PLE", "PNN", "TwoTower", "xDeepFM", "DataInputs",
           "DenseFeat", "FeatureDictionary", "MultiValCsvFeat", "ResilientLabelEncoder", "SequenceFeat", "SparseFeat", "SparseValueFeat",
           "hparams", "layers"]
