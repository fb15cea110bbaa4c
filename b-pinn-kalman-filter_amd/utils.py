"""Checkpoint I/O and small helpers (reference utils.py:1-128).

Checkpoint format is the reference's, so checkpoints move both ways:
  score models  {'info': 1, 'optimizer', 'model', 'ema', 'step'}
  PINN          {'info': 0, 'optimizer_1', 'optimizer_2', 'model', 'ema', 'step'}
Score-model state dicts carry the `module.` prefix of the reference's DataParallel
wrapper (models.utils.create_model keeps it).  Loading uses torch.load(weights_only=True):
the files hold only tensors, numbers and containers, so nothing is unpickled beyond data.
"""
from __future__ import annotations

import logging
import os
import time

import torch


class Clock:
    """Prints `info` at most every `itv` seconds (reference utils.py:7-19)."""

    def __init__(self, itv):
        self.itv = itv
        self.start = time.time()

    def tic(self, info: str):
        if time.time() - self.start >= self.itv:
            print(info)
            self.start = time.time()


def show_memory_usage(device):
    print(f"Allocated memory: {torch.cuda.memory_allocated(device) / 1024 ** 2:.2f} MB")
    print(f"Reserved memory: {torch.cuda.memory_reserved(device) / 1024 ** 2:.2f} MB")


def get_ckptdir(workdir, ckpt="checkpoints", ckpt_meta="checkpoints-meta"):
    checkpoint_dir = os.path.join(workdir, ckpt)
    checkpoint_meta_dir = os.path.join(workdir, ckpt_meta, "checkpoint.pth")
    os.makedirs(checkpoint_dir, exist_ok=True)
    os.makedirs(os.path.dirname(checkpoint_meta_dir), exist_ok=True)
    return checkpoint_dir, checkpoint_meta_dir


def _load(path, device):
    return torch.load(path, map_location=device, weights_only=True)


def restore_checkpoint(ckpt_dir, state, device):
    """Resume `state` in place from a checkpoint file; missing file -> state unchanged
    (reference utils.py:39-60, model loaded with strict=False as there)."""
    if not os.path.exists(ckpt_dir):
        os.makedirs(os.path.dirname(ckpt_dir) or ".", exist_ok=True)
        logging.warning(f"No checkpoint found at {ckpt_dir}. Returned the same state as input")
        return state
    loaded = _load(ckpt_dir, device)
    if loaded["info"] == 0:
        state["model"].load_state_dict(loaded["model"], strict=False)
        state["ema"].load_state_dict(loaded["ema"])
        state["step"] = loaded["step"]
        state["optimizer"][0].load_state_dict(loaded["optimizer_1"])
        state["optimizer"][1].load_state_dict(loaded["optimizer_2"])
    else:
        state["optimizer"].load_state_dict(loaded["optimizer"])
        state["model"].load_state_dict(loaded["model"], strict=False)
        state["ema"].load_state_dict(loaded["ema"])
        state["step"] = loaded["step"]
    return state


def load_checkpoint(ckpt_dir, model, device):
    """Model weights only, strict (reference utils.py:98-106)."""
    if not os.path.exists(ckpt_dir):
        logging.warning(f"No checkpoint found at {ckpt_dir}. Returned the same state as input")
        return model
    model.load_state_dict(_load(ckpt_dir, device)["model"])
    return model


def restore_bpinn_checkpoint(pinn_ckpt_dir, bpinn_ckpt_dir, state, config):
    """Resume a B-PINN run (reference utils.py:62-92): from `bpinn_ckpt_dir` if it exists (the
    state's B_PINN, both optimizers, EMA and step are loaded in place); else from a trained
    deterministic PINN at `pinn_ckpt_dir` -- a fresh B_PINN initialised by MOPED from it and two
    new optimizers replace state['model'] / state['optimizer']; else the state is returned
    unchanged."""
    if os.path.exists(bpinn_ckpt_dir):
        loaded = _load(bpinn_ckpt_dir, config.device)
        state["optimizer"][0].load_state_dict(loaded["optimizer_1"])
        state["optimizer"][1].load_state_dict(loaded["optimizer_2"])
        state["model"].load_state_dict(loaded["model"], strict=False)
        state["ema"].load_state_dict(loaded["ema"])
        state["step"] = loaded["step"]
        return state
    if not os.path.exists(pinn_ckpt_dir):
        logging.warning(f"No B-PINN checkpoint at {bpinn_ckpt_dir} and no PINN checkpoint at "
                        f"{pinn_ckpt_dir}: state left as it is")
        return state
    import losses
    from pinn_kalman import pinn
    pretrained = load_checkpoint(pinn_ckpt_dir, pinn.PINN(config), config.device)
    model = pinn.B_PINN(config, pretrained)
    state["model"] = model
    state["optimizer"] = (
        losses.get_optimizer(config, model.flownet.parameters(), is_bpinn=True),
        losses.get_optimizer(config, model.pressurenet.parameters(), is_bpinn=True, lr_mul=.05))
    logging.warning(f"B-PINN initialised by MOPED from the PINN checkpoint {pinn_ckpt_dir}")
    return state


def save_checkpoint(ckpt_dir, state):
    if isinstance(state["optimizer"], tuple):
        saved = {"info": 0, "optimizer_1": state["optimizer"][0].state_dict(),
                 "optimizer_2": state["optimizer"][1].state_dict(),
                 "model": state["model"].state_dict(), "ema": state["ema"].state_dict(),
                 "step": state["step"]}
    else:
        saved = {"info": 1, "optimizer": state["optimizer"].state_dict(),
                 "model": state["model"].state_dict(), "ema": state["ema"].state_dict(),
                 "step": state["step"]}
    torch.save(saved, ckpt_dir)
