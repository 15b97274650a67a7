from .categorical import (ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS, AtomEncoder, BondEncoder, CategoricalEncoder)
from .lappe import LapPENodeEncoder
from .rwse import RWSENodeEncoder
from .signnet import GIN, MLP, GINConv, GINDeepSigns, MaskedGINDeepSigns, SignNetNodeEncoder

__all__ = ["GIN", "MLP", "GINConv", "GINDeepSigns", "MaskedGINDeepSigns", "SignNetNodeEncoder", "RWSENodeEncoder",
           "LapPENodeEncoder", "CategoricalEncoder", "AtomEncoder", "BondEncoder", "ATOM_FEATURE_DIMS", "BOND_FEATURE_DIMS"]
