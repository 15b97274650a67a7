"""The hscn_*_supported functions whose answer ends in an LDS limit, held row for row to
tests/golden/lds_envelopes.npz (tools/record_lds_envelopes.py: recorded from the commit before the launch sites shared
one helper and the limits one name).  No launch: runs without a GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lds_envelopes.npz")
# function: its argument names (a fixture row: these, then the answer)
ARGS = {
    "hscn_scn_resident_supported": ("F", "H", "K", "max_n", "max_e"),
    "hscn_scn_resident_train_step_supported": ("F", "H", "K", "max_n", "max_e"),
    "hscn_mpnn_supported": ("F", "H", "L", "C", "max_n", "max_ell"),
    "hscn_vl_supported": ("F", "H", "L", "C", "max_n", "max_v", "max_ell", "max_evv"),
    "hscn_signnet_supported": ("model", "use_bn", "F", "K", "hidden", "phi_out", "layers", "post_layers", "dim_pe",
                               "dim_x", "max_n", "max_e"),
}
FUNCTIONS = tuple(ARGS)


def test_the_fixture_straddles_every_limit():
    z = np.load(GOLDEN)
    assert sorted(z.files) == sorted(FUNCTIONS)
    for name in FUNCTIONS:
        r = z[name]
        width = r[:, 4] if name == "hscn_signnet_supported" else r[:, 1]          # hidden / H
        n_at = list(ARGS[name]).index("max_n")
        assert set(width.tolist()) in ({16, 32, 24}, {16, 32, 65})
        assert not r[(width != 16) & (width != 32), -1].any(), name               # the refused width
        for w in (16, 32):
            for per_node in (2, 8):
                g = r[(width == w) & (r[:, n_at + (2 if name == "hscn_vl_supported" else 1)] == per_node * r[:, n_at])
                      & (r[:, n_at] > 0)]
                if name.startswith("hscn_scn"):
                    g = g[g[:, 2] == 4]                                             # K = 64 is outside the step's widths
                ok = g[g[:, -1] == 1][:, n_at]
                assert len(ok) and ok.max() + 1 in g[g[:, -1] == 0][:, n_at], (name, w, per_node)


def test_envelopes_answer_as_recorded():
    from graph_hscn import _hip
    lib = _hip.lib()
    z = np.load(GOLDEN)
    for name in FUNCTIONS:
        fn = getattr(lib, name)
        r = z[name]
        assert r.shape[1] == len(ARGS[name]) + 1
        got = np.array([fn(*(int(v) for v in row[:-1])) for row in r], dtype=np.int32)
        bad = np.nonzero(got != r[:, -1])[0]
        assert len(bad) == 0, (name, dict(zip(ARGS[name], r[bad[0], :-1].tolist())), int(got[bad[0]]))
