"""train.EarlyStopping: the stop rule ``train.train`` and ``train_resident.fit_resident`` share (reference
train/train.py:196-211), on scripted validation losses, against ``train.train`` itself driven with stand-in epoch
functions over the same sequence (no GPU)."""
import pytest
import torch

# (validation losses per epoch, patience, min_delta, epochs that run) -- worked out by hand from the reference's rule
CASES = {
    # best 1.0, 0.9; then two evaluations without improvement
    "patience_of_two": ([1.0, 0.9, 0.95, 0.96, 0.5, 0.4], 2, 0.0, 4),
    # 0.95 and 0.91 do improve on 1.0, but not by more than min_delta
    "improvement_smaller_than_min_delta": ([1.0, 0.95, 0.91, 0.3], 2, 0.1, 3),
    "the_same_losses_without_min_delta": ([1.0, 0.95, 0.91, 0.3], 2, 0.0, 4),
    # stale reaches the patience at epoch 2: the last epoch of this run, but not of the next one
    "patience_reached_on_the_last_epoch_does_not_stop": ([1.0, 1.1, 1.2], 2, 0.0, 3),
    "the_same_losses_with_an_epoch_to_go": ([1.0, 1.1, 1.2, 0.1], 2, 0.0, 3),
    "an_improvement_rewinds_the_count": ([1.0, 1.1, 0.8, 0.9, 0.7, 0.9, 0.9, 0.1], 2, 0.0, 7),
    "never_stale": ([1.0, 0.9, 0.8, 0.7], 1, 0.0, 4),
}


def _cfg(losses, patience, min_delta):
    from graph_hscn.config.config import TrainingConfig
    return TrainingConfig("hscn", "cross_entropy", "ap", epochs=len(losses), eval_period=1, min_delta=min_delta,
                          patience=patience)


def _helper_epochs(losses, patience, min_delta):
    from graph_hscn.train.train import EarlyStopping
    stopper = EarlyStopping(_cfg(losses, patience, min_delta))
    for epoch, loss in enumerate(losses):
        if stopper.update(loss, epoch):
            return epoch + 1
    return len(losses)


def _train_epochs(losses, patience, min_delta, monkeypatch):
    """The number of epochs ``train.train`` runs when the validation loss of epoch e is ``losses[e]``."""
    from graph_hscn.config.config import OptimConfig
    from graph_hscn.train import train as T
    evaluated = []

    def train_epoch(epoch, *a, **kw):
        return 0.0, float("nan")

    def eval_epoch(epoch, logger, loader, model, loss_fn, metric_fn, split):
        evaluated.append((epoch, split))
        return (losses[epoch] if split == "Validation" else 123.0), float("nan")

    monkeypatch.setattr(T, "train_epoch", train_epoch)
    monkeypatch.setattr(T, "eval_epoch", eval_epoch)
    history = T.train(None, OptimConfig("adam", lr=0.01), _cfg(losses, patience, min_delta), [[], [], []],
                      torch.nn.Linear(2, 1))
    ran = len(history)
    stopped = ran < len(losses)      # (the test split of the stopping epoch is not evaluated, as in the reference)
    assert [e for e, s in evaluated if s == "Validation"] == list(range(ran))
    assert [e for e, s in evaluated if s == "Test"] == list(range(ran - 1 if stopped else ran))
    return ran


@pytest.mark.parametrize("case", sorted(CASES))
def test_helper_stops_where_train_stops(case, monkeypatch):
    losses, patience, min_delta, want = CASES[case]
    assert _helper_epochs(losses, patience, min_delta) == want
    assert _train_epochs(losses, patience, min_delta, monkeypatch) == want


def test_a_reducer_of_one_rank_issues_no_collective():
    """Only several ranks have anything to agree on: a world of one must not need a process group."""
    from graph_hscn.train.train import EarlyStopping

    class Reducer:
        world_size, group = 1, None

    stopper = EarlyStopping(_cfg([1.0, 2.0, 3.0], 1, 0.0), Reducer(), "cpu")
    assert [stopper.update(loss, e) for e, loss in enumerate([1.0, 2.0, 3.0])] == [False, True, False]
