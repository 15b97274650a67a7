"""The bar of tests/test_gpu_scn_resident_f64.py shown on the REFERENCE alone (no device, no launch): for every case of
its table

  * four held-out float32 evaluations of the CPU oracle on relabelled copies of the batch (``helpers.relabel_graphs``,
    seeds that are not among the yardstick's) -- correct float32 evaluations of the same gradients by construction --
    pass ``referee_all`` against the eight-draw yardstick:  |o32' - f64| <= 2 max_r |o32_r - f64| + 8 * 2^-23 max|f64|;
  * the same four are REJECTED by ``teeth`` against the float64 reference with one edge of the largest graph removed:
    the eight-draw bar is not blind;
  * the kink guard holds on the float64 oracle (asserted inside ``_references``; the ReLU cases' seeds were chosen for
    it);
  * ``hscn_scn_resident_supported`` / ``hscn_scn_resident_train_step_supported`` answer what the table writes down for
    the batch's own maxima, and the envelope limits it names are the queries' own.

If a case's held-out draws do not pass here, the seed or the case changes, never the bar.
"""
import pytest
import torch

from tests.helpers import most_changed, referee_all, relabel_graphs, teeth
from tests.test_gpu_layered_f64 import _oracle_eval
from tests.test_gpu_scn_resident_f64 import (CASES, HELD_OUT_SEEDS, YARDSTICK_SEEDS, _references_of, cotangent,
                                             supported, what_of)


@pytest.mark.parametrize("c", CASES)
def test_held_out_float32_evaluations_pass_the_eight_draw_bar_and_its_teeth(c):
    what = what_of(c) + " [reference only]"
    om, graphs, maxima, ref = _references_of(c["id"])
    print(f"[stage A referee, host] {what}: (max_n, max_e) = {maxima}")
    assert not set(HELD_OUT_SEEDS) & set(YARDSTICK_SEEDS)
    assert isinstance(ref["g32"], list) and len(ref["g32"]) == 1 + len(YARDSTICK_SEEDS)
    gy = cotangent(graphs, c["K"])
    reached = most_changed(ref["g64"], ref["dropped"]) if ref["dropped"] else {}
    if max(e.size(1) for _, e in graphs):
        assert reached, f"{what}: the dropped edge reaches no gradient"
    worst = 0.0
    for s in HELD_OUT_SEEDS:
        held = _oracle_eval(om, {}, {"graphs": relabel_graphs(graphs, s)}, gy, torch.float32)[1]
        worst = max(worst, referee_all(held, ref["g32"], ref["g64"], f"{what} held-out {s}"))
        teeth(held, ref["g32"], ref["g64"], reached, f"{what} held-out {s}")
    print(f"   worst held-out ratio of {what}: {worst:.3f}")


def test_a_list_of_draws_takes_the_largest_distance_and_one_tensor_is_unchanged():
    from tests.helpers import referee
    o64 = torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64)
    near, far = o64 + 1e-7, o64 - 3e-7
    got = o64 + 5e-7
    ulp = 2.0 ** -23 * 4.0
    one = referee(got, near, o64, "single")
    assert one == float((got - o64).abs().max()) / (2.0 * float((near.double() - o64).abs().max()) + 8.0 * ulp)
    assert referee(got, [near], o64, "list of one") == one
    both = referee(got, [near, far], o64, "two draws")
    assert both == referee(got, [far, near], o64, "two draws, other order") == referee(got, far, o64, "the farther one")
    assert both < one
    assert referee(got, [near, far[:2]], o64, "shape mismatch in a draw") == float("inf")


def test_a_relabelled_copy_is_the_same_batch():
    """``relabel_graphs``: the rows of x and the edges are the original's under the node permutation (checked through
    permutation-invariant sums in exact integer arithmetic), the float64 oracle's losses and gradients agree to float64
    rounding, and the float32 evaluation is a different draw."""
    c = CASES[6].values[0]                                     # the multigraph: repeats, loops, a hub, isolated nodes
    om, graphs, _, ref = _references_of(c["id"])
    copy_ = relabel_graphs(graphs, 5)
    for (x, ei), (x2, e2) in zip(graphs, copy_):
        assert x2.shape == x.shape and e2.shape == ei.shape and not torch.equal(e2, ei)
        n = x.size(0)
        key = x.long() @ (7 ** torch.arange(x.size(1)))          # one integer per node (features are 0 .. 4)
        key2 = x2.long() @ (7 ** torch.arange(x.size(1)))
        assert sorted(key.tolist()) == sorted(key2.tolist())
        pairs = sorted(zip(key[ei[0]].tolist(), key[ei[1]].tolist()))
        assert pairs == sorted(zip(key2[e2[0]].tolist(), key2[e2[1]].tolist()))
        assert sorted(torch.bincount(ei[1], minlength=n).tolist()) == sorted(torch.bincount(e2[1], minlength=n).tolist())
    gy = cotangent(graphs, c["K"])
    g64 = _oracle_eval(om, {}, {"graphs": copy_}, gy, torch.float64)[1]
    g32 = _oracle_eval(om, {}, {"graphs": copy_}, gy, torch.float32)[1]
    for k, v in ref["g64"].items():
        assert float((g64[k] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k
    assert any(not torch.equal(g32[k], ref["g32"][0][k]) for k in g32)


def _largest_n(fn, c, max_e, lo, hi=2048):
    args = (c["F"], c["H"], c["K"])
    ok = [n for n in range(lo, hi) if fn(*args, n, max_e)]
    assert ok and ok == list(range(lo, ok[-1] + 1)), "the envelope is an interval of max_n"
    return ok[-1]


@pytest.mark.parametrize("c", CASES)
def test_the_cases_lie_where_the_table_says(c):
    from graph_hscn import _hip
    lib = _hip.lib()
    _, graphs, maxima, _ = _references_of(c["id"])
    e = c["expect"]
    assert supported(c, maxima) == (e["pair"], e["step"]), (c["id"], maxima)
    if "step_max_n" in e:
        assert _largest_n(lib.hscn_scn_resident_train_step_supported, c, maxima[1], maxima[0]) == e["step_max_n"]
    if "pair_max_n" in e:
        assert _largest_n(lib.hscn_scn_resident_supported, c, maxima[1], maxima[0]) == e["pair_max_n"]
