"""``pre_transform_in_memory`` with the reference's contract (transform/pre_transform.py:7-25) for this package's
datasets, which are plain lists of ``Data``."""
from __future__ import annotations

from typing import Callable, List, Optional


def pre_transform_in_memory(dataset: List, transform_func: Optional[Callable], show_progress: bool = False):
    """``None`` transform: the dataset is returned.  Otherwise every graph is replaced IN PLACE by
    ``transform_func(graph)`` and graphs for which it returns ``None`` are removed (nothing is returned, as in the
    reference).  ``show_progress`` logs a line every twentieth of the dataset."""
    if transform_func is None:
        return dataset
    n = len(dataset)
    every = max(1, n // 20)
    out = []
    for i in range(n):
        g = transform_func(dataset[i])
        if g is not None:
            out.append(g)
        if show_progress and ((i + 1) % every == 0 or i + 1 == n):
            print(f"pre_transform_in_memory: {i + 1} / {n}", flush=True)
    dataset[:] = out
    return None
