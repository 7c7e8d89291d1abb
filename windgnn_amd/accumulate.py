"""The arithmetic of TrainStep.accumulate / accumulate_series / apply (trainer.py): several calls' final gradient buckets
become the bucket of ONE call on the union of their windows.  Plain torch on the current stream, no host read, no kernel of
the library (DESIGN.md §5 "Accumulating gradients over several calls"); CPU tensors work as well, which is how
tests/test_accumulate_host.py checks it against fp64.

Call i leaves its bucket b_i = [header with the loss word l_i | gradients g_i], the gradient of ITS mean loss over ITS c_i counted
labels.  The mean loss over all C = sum c_i labels is sum (c_i / C) l_i, and so is its gradient.  The accumulator holds

    acc = sum (c_i / c_1) b_i        (header and gradients alike: one buffer of the bucket's size)        C = sum c_i

and `write` leaves acc * (c_1 / C) in the bucket.  Normalising by the FIRST call's count, not by C (unknown until apply) and not
at all (c_i b_i overflows nothing, but one call would then be scaled by c_1 and back by 1 / c_1, two roundings), makes one call
alone exact: the first add is a copy, c_1 / C = 1.0, and x * 1.0 = x, so accumulate + apply reproduces the bucket bit for bit.

A count is a host integer (windows x counted steps x outputs) or a 0-dim integer device tensor (labels that exist, under
missing_labels).  Either way the weight reaches the buffer as a 0-dim fp32 tensor, float32(float64(c_i) / float64(c_1)), through
the same torch.addcmul: host integers are divided in Python (the same IEEE division) and filled into a device scalar, so a
device count and the host integer of the same value give the same bits.  Once a device count has entered, C and c_1 are known on
the device only and every later weight is formed there."""
from __future__ import annotations

import torch


def _weight(num, den, device):
    """float32(float64(num) / float64(den)) as a 0-dim tensor on `device`: in Python for two host integers, else on the device."""
    if not torch.is_tensor(num) and not torch.is_tensor(den):
        return torch.full((), num / den if den else float("nan"), dtype=torch.float32, device=device)
    num = num.to(torch.float64) if torch.is_tensor(num) else torch.full((), float(num), dtype=torch.float64, device=device)
    return (num / den).to(torch.float32)          # (c / 0 = inf or NaN: a first call without a single label poisons the step)


class Accumulation:
    """The open accumulation over a bucket of `like`'s size and layout.  `calls`: the calls added since the last reset (a host
    int); `count`: C as a 0-dim int64 view on the device."""

    def __init__(self, like: torch.Tensor):
        self.buf = torch.zeros_like(like)
        self._words = torch.zeros(2, dtype=torch.int64, device=like.device)        # C, c_1
        self.calls = 0
        self._host = None           # (C, c_1) as host integers while every count so far was one, else None

    @property
    def count(self) -> torch.Tensor:
        return self._words[0]

    def reset(self) -> None:
        """Drop what was added (nothing is launched: the next add overwrites the buffer and the words)."""
        self.calls, self._host = 0, None

    def add(self, bucket: torch.Tensor, count) -> None:
        """acc += (count / c_1) * bucket and C += count; the first add of an accumulation is the copy (weight 1 by
        definition).  The host state changes last: an add that raises leaves the accumulation's bookkeeping as it was."""
        on_device = torch.is_tensor(count)
        if on_device:
            count = count.reshape(()).to(torch.int64)
        else:
            count = int(count)
        if self.calls == 0:
            self.buf.copy_(bucket)
            if on_device:
                self._words.copy_(count.expand(2))
            else:
                self._words.fill_(count)
            self.calls, self._host = 1, None if on_device else (count, count)
            return
        host = self._host if not on_device else None
        w = _weight(count, host[1] if host is not None else self._words[1], bucket.device)
        self.buf.addcmul_(bucket, w)
        self._words[0] += count
        self.calls, self._host = self.calls + 1, (host[0] + count, host[1]) if host is not None else None

    def write(self, bucket: torch.Tensor, loss_slot: int, weight: float = 1.0) -> None:
        """bucket = acc * (c_1 / C) * weight, its loss word acc[loss_slot] * (c_1 / C): the gradient (times this shard's
        weight, which the exchange applies to the loss word itself) and the mean loss of one call on the union."""
        if self._host is not None:
            s = _weight(self._host[1], self._host[0], bucket.device)
        else:
            s = _weight(self._words[1], self._words[0], bucket.device)
        if weight == 1.0:
            torch.mul(self.buf, s, out=bucket)
            return
        torch.mul(self.buf, s * weight, out=bucket)
        torch.mul(self.buf[loss_slot], s, out=bucket[loss_slot])
