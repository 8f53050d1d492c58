"""Clouds of different sizes in one batch: the one statement of what the attacks' ragged passes share.

A ragged batch is [B, Kmax, 3] with one length per cloud; rows at and beyond a length are padding, copies of the cloud's row
0 (ops.pad_ragged). The lengths are device DATA of the launches, so one captured graph serves every set of lengths; a loop's
key carries the flag "ragged", never the lengths. What is here is host code: the lengths check, the seeded start draw, the
transfer prediction, the victim's lengths keyword and a device loop's lengths buffers.
"""
import numpy as np
import torch

from . import graphed as _graphed


def check_lengths(who, lengths, B, K, low=1, low_text="1", empty_ok=False):
    """lengths (sequence, array or tensor) as int64 numpy [B], or ValueError in `who`'s name: B ints, each in [low, K].
    low_text: how the caller spells `low` in its message ("1": a literal bound). An empty batch passes with empty_ok only."""
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().numpy()
    lens = np.asarray(lengths)
    if lens.shape != (B,) or not np.issubdtype(lens.dtype, np.integer):
        raise ValueError(f"{who}: lengths must be {B} ints, got shape {lens.shape} dtype {lens.dtype}")
    if B == 0:
        if not empty_ok:
            raise ValueError(f"{who}: lengths must not be empty (a batch of 0 clouds)")
        return lens.astype(np.int64)
    if lens.min() < low or lens.max() > K:
        spelled = low_text if low_text == str(low) else f"{low_text}={low}"
        raise ValueError(f"{who}: lengths must lie in [{spelled}, Kmax={K}], got [{lens.min()}, {lens.max()}]")
    return lens.astype(np.int64)


def per_cloud_draw(B, c, K, lens, draw):
    """The seeded start of a ragged batch, CPU [B, c, K]: row b holds draw(b, lens[b]) — shape [c, lens[b]], what a run of
    that cloud alone draws from the sample's own generator — in its first columns and zeros behind. draw is called once per
    cloud, in batch order."""
    out = torch.zeros((B, c, K))
    for b in range(B):
        n = int(lens[b])
        out[b, :, :n] = draw(b, n)
    return out


def predict(model, x, lens=None):
    """The labels `model` gives x [B,3,K]. lens (a ragged batch's sizes): a model that declares pad_invariant sees the padded
    batch, any other every cloud alone, on its own [1,3,lens[b]] slice (B forwards, once per attack)."""
    if lens is None or getattr(_graphed.unwrap(model), "pad_invariant", False):
        return torch.argmax(_graphed.logits_of(model(x)), dim=1)
    return torch.cat([torch.argmax(_graphed.logits_of(model(x[b:b + 1, :, :int(n)].contiguous())), dim=1)
                      for b, n in enumerate(lens)])


def victim_kwargs(victim, lens_dev):
    """The keywords a ragged pass adds to the victim's fused entry points: the lengths for a victim that declares
    fused_lengths (its towers then skip the padding), nothing for any other (pad_invariant: it sees the padded batch, the
    padding rows' gradient is exactly zero either way) and nothing for a dense pass (lens_dev None)."""
    if lens_dev is not None and getattr(_graphed.unwrap(victim), "fused_lengths", False):
        return dict(lengths=lens_dev)
    return {}


def loop_lengths(B, K, dev):
    """(lens int32 [B] on dev, lens_host int64 numpy [B]) of a ragged device loop: the buffer the captured launches read and
    the host copy the search wrapper checks. Both start at K, the dense batch; every call overwrites them
    (set_loop_lengths) before any pass runs."""
    return torch.full((B,), K, dtype=torch.int32, device=dev), np.full((B,), K, dtype=np.int64)


def set_loop_lengths(bufs, lens):
    """A call's lengths (int64 numpy [B]) into the loop's two buffers, in place: the graphs point at them."""
    bufs["lens_host"][:] = lens
    bufs["lens"].copy_(torch.from_numpy(lens.astype(np.int32)))
