"""train_resident.optimizer_steps_at: the stepping rule of the captured loop is train.train_epoch's (reference
train/train.py:89: every k-th batch and always the last one), checked against train_epoch itself on the CPU
with a stand-in model, optimizer and criterion (no GPU)."""
import pytest
import torch


class _Batch:
    def __init__(self, i):
        self.x = torch.full((1, 2), float(i))
        self.y = torch.zeros(1, 1)

    def to(self, device):
        return self


class _CountingOptimizer:
    def __init__(self, params, log):
        self.params = list(params)
        self.log = log
        self.it = None

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        self.log.append(self.it)


def _train_epoch_steps(num_batches, k, monkeypatch):
    """The iterations at which train.train_epoch steps its optimizer on an epoch of ``num_batches`` batches."""
    from graph_hscn.train import train as T
    lin = torch.nn.Linear(2, 1)
    log = []
    opt = _CountingOptimizer(lin.parameters(), log)
    batches = [_Batch(i) for i in range(num_batches)]

    def crit(loss_fn, pred, true):
        return ((pred - true) ** 2).mean(), pred

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = lin

        def forward(self, batch):
            opt.it = int(batch.x[0, 0])          # the iteration the next step() belongs to
            return self.lin(batch.x)

    model = Model()

    monkeypatch.setattr(T, "criterion", crit)
    T.train_epoch(0, None, batches, model, opt, "l1", None, k, False)
    return log


@pytest.mark.parametrize("k", range(1, 7))
def test_stepping_rule_matches_train_epoch(k, monkeypatch):
    from graph_hscn.train.train_resident import optimizer_steps_at
    for num_batches in range(1, 21):
        want = _train_epoch_steps(num_batches, k, monkeypatch)
        got = [it for it in range(num_batches) if optimizer_steps_at(it, num_batches, k)]
        assert got == want, (num_batches, k)
        # an epoch of `steps` captured batches, with and without the eager tail batch that fit_resident counts as the
        # last iteration: the tail always steps, and the captured batches step as train_epoch's do
        for steps, tail in ((num_batches, 0), (num_batches - 1, 1)):
            if steps < 1:
                continue
            n = steps + tail
            assert [i for i in range(steps) if optimizer_steps_at(i, n, k)] == [i for i in want if i < steps]
            if tail:
                assert optimizer_steps_at(steps, n, k)


def test_every_window_ends_in_a_step():
    from graph_hscn.train.train_resident import optimizer_steps_at
    for k in range(1, 7):
        for n in range(1, 21):
            steps = [it for it in range(n) if optimizer_steps_at(it, n, k)]
            assert steps[-1] == n - 1
            assert len(steps) == (n + k - 1) // k
            gaps = [b - a for a, b in zip([-1] + steps, steps)]
            assert all(1 <= g <= k for g in gaps)
