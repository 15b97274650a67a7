from .categorical import (ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS, AtomEncoder, BondEncoder, CategoricalEncoder)
from .rwse import RWSENodeEncoder
from .signnet import GIN, MLP, GINConv, GINDeepSigns, MaskedGINDeepSigns, SignNetNodeEncoder

__all__ = ["GIN", "MLP", "GINConv", "GINDeepSigns", "MaskedGINDeepSigns", "SignNetNodeEncoder", "RWSENodeEncoder",
           "CategoricalEncoder", "AtomEncoder", "BondEncoder", "ATOM_FEATURE_DIMS", "BOND_FEATURE_DIMS"]
