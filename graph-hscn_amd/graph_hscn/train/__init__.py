from .train import compute_posenc, get_each_data_from_batch, is_eval_epoch

__all__ = ["compute_posenc", "get_each_data_from_batch", "is_eval_epoch"]
