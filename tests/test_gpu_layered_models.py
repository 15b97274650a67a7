"""GPS, SAN and GCNII on the device across the change that gave them one base class (model/_common.py LayeredModel):

  * an ``eval()`` forward of each gives the bits it gave on the commit before the base existed
    (tests/golden/layered_models_parent_outputs.json, written by ``record_parent_outputs`` on that commit): the
    kernels involved use no float atomics and repeat their bits, so equality is asked for, not a tolerance;
  * the graph-level mean pool of all three is the column-sliced one GCNII had: GPS and SAN at 320 columns under the
    float64 referee and the cut of tests/test_gpu_gcn2.py, and one graph-level forward and backward of each."""
import json
import os

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import Batch
from graph_hscn.model.gcnii import GCNII
from graph_hscn.model.gps import GPS
from graph_hscn.model.san import SAN
from graph_hscn.nn.conv import Linear
from tests.helpers import DEV, referee_all, teeth
from tests.test_gpu_gcn2 import M_C, M_F, M_SIZES, _model_batch, _peptides, _pool_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layered_models_parent_outputs.json")
SEED = 4321
RELU = ACT_DICT["relu"]
EQUIVALENCE = {
    "gps": lambda: GPS(9, 32, 10, 2, 4, "gine", RELU),
    "san": lambda: SAN(9, 32, 10, 2, 4, RELU, node_encoder="atom", edge_encoder="bond"),
    "gcnii": lambda: GCNII(9, 32, 10, 3, RELU),
}


def _eval_forward(name):
    """[8, 10] float32 on the host: the model built under SEED on the CPU -- a ``Linear(-1, D)`` over the three bond
    columns drawn there too, so that no value depends on the device's generator -- on eight Peptides-shaped graphs."""
    from graph_hscn.train import batching
    torch.manual_seed(SEED)
    m = EQUIVALENCE[name]()
    for mod in m.modules():
        if isinstance(mod, Linear):
            mod.materialize(3, torch.empty(0))
    m = m.to(DEV).eval()
    bd = batching.to_device(m, Batch.from_data_list(_peptides()), DEV)
    with torch.no_grad():
        out = m(bd)
    m.check_flags()
    assert m.last_engine == "layered" and out.dtype == torch.float32 and tuple(out.shape) == (8, 10)
    return out.cpu()


def _bits(t):
    return np.ascontiguousarray(t.numpy(), dtype=np.float32).view(np.int32)


def record_parent_outputs():
    """What wrote the golden file, run on the commit before ``LayeredModel`` existed: each output's float32 bit
    patterns, twice over to say whether the run repeats its bits."""
    res = {"seed": SEED}
    for name in EQUIVALENCE:
        first, again = _bits(_eval_forward(name)), _bits(_eval_forward(name))
        res[name] = {"bits": first.tolist(), "repeats": bool(np.array_equal(first, again))}
    return res


@pytest.mark.parametrize("name", list(EQUIVALENCE))
def test_an_eval_forward_gives_the_bits_it_gave(name):
    want = json.load(open(GOLDEN))
    assert want["seed"] == SEED and want[name]["repeats"] is True
    got = _eval_forward(name)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 1e-3
    assert np.array_equal(_bits(got), np.asarray(want[name]["bits"], dtype=np.int32))


WIDE = 320                                                      # five heads of the widest kind: above the pool's 256
WIDE_MODELS = {
    "gps": lambda: GPS(M_F, WIDE, M_C, 1, num_heads=5, local_conv=None),
    "san": lambda: SAN(M_F, WIDE, M_C, 1, num_heads=5),
    "gcnii": lambda: GCNII(M_F, WIDE, M_C, 1),
}


@pytest.mark.parametrize("name", list(WIDE_MODELS))
def test_the_graph_level_pools_320_columns_in_slices(name):
    from graph_hscn.model.gcnii import POOL_MAX_WIDTH
    from graph_hscn.train import batching
    assert POOL_MAX_WIDTH < WIDE < 2 * POOL_MAX_WIDTH
    b, x, gy, o32, o64 = _pool_reference(WIDE)
    pm = WIDE_MODELS[name]().to(DEV)
    bd = batching.to_device(pm, b, DEV)
    t = x.clone().to(DEV).requires_grad_(True)
    out = pm._pool(t, bd)
    out.backward(gy.to(DEV))
    what = f"{name}'s mean pool at H={WIDE}"
    referee_all({"pooled": out, "g_x": t.grad}, o32, o64, what)
    o64_cut = {"pooled": o64["pooled"].clone()}
    o64_cut["pooled"][4, WIDE - 1] -= x[int(b.ptr[4]), WIDE - 1].double() / M_SIZES[4]   # one node of the last column left out
    teeth({"pooled": out}, o32, o64, o64_cut, what)


@pytest.mark.parametrize("name", ["gps", "san"])
def test_a_wide_graph_level_model_runs_forward_and_backward(name):
    from graph_hscn.train import batching
    torch.manual_seed(7)
    pm = WIDE_MODELS[name]().to(DEV)
    bd = batching.to_device(pm, _model_batch(0, "linear", "graph"), DEV)
    out = pm(bd)
    out.sum().backward()
    pm.check_flags()
    assert tuple(out.shape) == (len(M_SIZES), M_C) and bool(torch.isfinite(out).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in pm.parameters() if p.grad is not None)
    assert bool(pm.node_encoder.weight.grad.any())              # the pooled columns carry the gradient back
