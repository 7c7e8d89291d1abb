"""Several models trained at once: K TrainSteps on a few side streams of one device, their forecasts as mean and spread.

What a user does with a model of this size is run many of them -- seeds for an ensemble, folds of a rolling-origin
cross-validation (series.kfold_starts), a sweep over lr / max_grad_norm / the loss -- and a step on a few hundred windows leaves
most of the device idle (the recurrences launch n / 16 workgroups).  Ensemble issues the members' steps on `streams` side
streams, so that the device may run them side by side.  No kernel and no entry point of the library is added: the hot path is
the members' own step kernels, each member is a TrainStep as it is alone (bit for bit: the kernels are bit-reproducible, their
split-K plans depend on the dims alone, and functional._Workspace keeps one scratch per stream), and the only new device work is
the [K, n, 3S] reduction of a forecast (torch operations in fp64).  DESIGN.md section 5, "Ensembles: members on streams".

Every fan-out call (step, step_series, validate, validate_series, forward_backward, forward_backward_series, restore_best, each
and the forecasts) follows one discipline:

  1. an event recorded on the caller's current stream is waited on by every side stream in use;
  2. members are issued in order k = 0 .. K - 1, each member's WHOLE call with side[k % streams] as torch's current stream
     (what `with torch.cuda.stream(...)` sets): two members that share a stream never interleave (a deferred backward keeps its partial sums live in that stream's workspace
     until its wgnn_finish);
  3. every side stream in use records an event and the caller's stream waits on it.

To the caller the call is one call on their current stream: inputs may arrive late on it, results are ordered on it, and nothing
synchronises with the host.  Tensors a member hands back were allocated under its side stream; record_stream marks them for
the caller's stream, so that the caching allocator does not give their memory out again while the caller still reads it.

More side streams than the process has hardware queues (HIP's default is 4; the environment variable GPU_MAX_HW_QUEUES sets it,
and this module sets nothing) share queues: their work is then serialised as on one stream, in an order the runtime picks.

The members' periodic range check (TrainStep(check_every=)) does not run inside a member's call -- check_range_status reads the
status word of every workspace of the process, which would wait for the other members' streams in mid-flight -- but from the
ensemble after the join, whenever a member's `steps` has passed a multiple of check_every; its message names the members of the
stream whose workspace reported.

Out of scope: collectives from several streams (process_group, direct_rccl, overlap_collectives, grad_blocks are refused), one
issuing host thread per stream, K models in one launch, weighted or stacked combination, graph capture."""
from __future__ import annotations

import collections

import torch

from . import _lib
from . import functional as _F
from .modules import GCN_GRU
from .series import _upload, n_series_windows
from .trainer import TrainStep

DEFAULT_STREAMS = 4                 # HIP's default number of hardware queues per process
_COLLECTIVE_KEYWORDS = ("process_group", "direct_rccl", "overlap_collectives", "grad_blocks")

EnsembleForecast = collections.namedtuple("EnsembleForecast", "mean std members")


class PerMember:
    """A marker around a length-K sequence: in any Ensemble call an argument wrapped in it is handed out member by member
    (member k gets seq[k]); every other argument is shared by all members."""

    def __init__(self, seq):
        self.seq = list(seq)

    def __len__(self):
        return len(self.seq)

    def __getitem__(self, k):
        return self.seq[k]

    def __repr__(self):
        return "PerMember(%r)" % (self.seq,)


class _Cuda:
    """The stream operations of the fan-out, in one place (tests/test_ensemble_host.py replaces them by recorders)."""

    @staticmethod
    def new_stream(device):
        return torch.cuda.Stream(device)

    @staticmethod
    def current_stream(device):
        return torch.cuda.current_stream(device)

    @staticmethod
    def event():
        return torch.cuda.Event()

    @staticmethod
    def set_stream(stream):
        """What torch.cuda.stream(stream) does on entry and, with the previous stream, on exit (the context manager itself
        costs the host several microseconds per member)."""
        torch.cuda.set_stream(stream)

    @staticmethod
    def hand_back(t, stream):
        if t.is_cuda:
            t.record_stream(stream)


_cuda = _Cuda


def _hand_back(out, stream):
    """record_stream on every tensor of a member's return value (tensors, tuples / lists of them)."""
    if torch.is_tensor(out):
        _cuda.hand_back(out, stream)
    elif isinstance(out, (tuple, list)):
        for o in out:
            _hand_back(o, stream)


def mean_std(members: torch.Tensor):
    """(mean, std) over dim 0 of members [K, n, C] (fp32): both formed in fp64 from the fp32 members and rounded once to fp32;
    std is the population spread sqrt(mean((x - mean)^2)), so K = 1 gives zeros.  Rows are taken in chunks that keep one fp64
    temporary (K * C * 8 bytes per row) under functional.validation_chunk_windows' 64 MiB.  Plain torch on the current stream,
    no host read; CPU tensors work as well."""
    if members.dim() != 3 or members.shape[0] < 1:
        raise ValueError("windgnn_amd: mean_std wants members [K >= 1, n, C], got %s" % (tuple(members.shape),))
    K, n, C = members.shape
    mean = torch.empty(n, C, dtype=torch.float32, device=members.device)
    std = torch.empty_like(mean)
    step = _F.validation_chunk_windows(n, K, C) if n else 1
    for r0 in range(0, n, step):
        x = members[:, r0:r0 + step].to(torch.float64)
        m = x.mean(dim=0)
        mean[r0:r0 + step] = m
        x -= m
        std[r0:r0 + step] = x.square_().mean(dim=0).sqrt_()
    return mean, std


class _BestOf:
    """What the forecast functions read of a model -- fused, math, hot_path_parameters() -- on a TrainStep's best snapshot."""

    def __init__(self, tr):
        self.fused, self.math, self._views = tr.model.fused, tr.model.math, tr._best_views

    def hot_path_parameters(self):
        return self._views


class Ensemble:
    def __init__(self, models, *, streams=None, **trainstep_kwargs):
        """models: K fused GCN_GRU on one device; one TrainStep per member is built from trainstep_kwargs, each of which is a
        scalar (shared) or a PerMember (a sweep: lr=PerMember([...]), max_grad_norm=PerMember([None, 1.0, inf]),
        keep_best=...).  streams: the side streams, min(K, 4) by default (module docstring); member k runs on
        side[k % streams].  check_every (default 100, shared): the ensemble's own range check after the join.
        Refused by name: process_group, direct_rccl, overlap_collectives, grad_blocks; members on different devices; a
        PerMember whose length is not K; streams < 1."""
        models = list(models)
        K = len(models)
        if K < 1:
            raise ValueError("windgnn_amd: Ensemble(models): at least one model, got none")
        for name in _COLLECTIVE_KEYWORDS:
            if name in trainstep_kwargs:
                raise RuntimeError("windgnn_amd: Ensemble(%s=...): collectives issued from several streams are a follow-up that is "
                                   "not built; an Ensemble trains its members on one device without a process group (data "
                                   "parallel: one TrainStep per rank)" % name)
        for name, value in trainstep_kwargs.items():
            self._check_len("Ensemble", name, value, K)
        if isinstance(trainstep_kwargs.get("check_every"), PerMember):
            raise ValueError("windgnn_amd: Ensemble(check_every=PerMember(...)): the range check runs from the ensemble after the "
                             "join, once for all members; pass one value")
        if streams is None:
            streams = min(K, DEFAULT_STREAMS)
        if int(streams) != streams or int(streams) < 1:
            raise ValueError("windgnn_amd: Ensemble(streams=%r): at least one side stream (default min(K, %d))"
                             % (streams, DEFAULT_STREAMS))
        devices = []
        for k, m in enumerate(models):
            if not isinstance(m, GCN_GRU):
                raise TypeError("windgnn_amd: Ensemble(models): models[%d] is %s, not a windgnn_amd.GCN_GRU" % (k, type(m).__name__))
            devices.append(next(m.parameters()).device)
        if len(set(devices)) != 1:
            raise RuntimeError("windgnn_amd: Ensemble(models): the members must be on one device, got %s (members on several "
                               "devices are K independent TrainSteps)" % ", ".join("models[%d] on %s" % kd for kd in enumerate(devices)))
        self.K, self.device, self.n_streams = K, devices[0], int(streams)
        self.check_every = int(trainstep_kwargs.pop("check_every", 100))
        # (check_every=0: a member never reads the status words from inside its side-stream call; _check_after does)
        self.members = [TrainStep(m, check_every=0, **{n: self._pick(v, k) for n, v in trainstep_kwargs.items()})
                        for k, m in enumerate(models)]
        self.side = [_cuda.new_stream(self.device) for _ in range(self.n_streams)]
        # the fork's and the joins' events, made once (a wait takes the record that precedes it, so they are reused)
        self._fork, self._done = _cuda.event(), [_cuda.event() for _ in range(self.n_streams)]

    # ---- arguments ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_len(who, name, value, K):
        if isinstance(value, PerMember) and len(value) != K:
            raise ValueError("windgnn_amd: %s: %s=PerMember(...) holds %d entries for %d members" % (who, name, len(value), K))

    @staticmethod
    def _pick(value, k):
        return value[k] if isinstance(value, PerMember) else value

    def _resolve(self, who, names, args, kwargs):
        """Member k's (args, kwargs) for k = 0 .. K - 1; a PerMember of another length is refused here, before any call."""
        for i, a in enumerate(args):
            self._check_len("Ensemble." + who, names[i] if i < len(names) else "argument %d" % i, a, self.K)
        for n, a in kwargs.items():
            self._check_len("Ensemble." + who, n, a, self.K)
        return [(tuple(self._pick(a, k) for a in args), {n: self._pick(a, k) for n, a in kwargs.items()}) for k in range(self.K)]

    def stream_of(self, k):
        """The side stream member k runs on."""
        return self.side[k % self.n_streams]

    def members_of(self, s):
        """The members that run on side stream s."""
        return [k for k in range(self.K) if k % self.n_streams == s]

    # ---- the fan-out ----------------------------------------------------------------------------------------------------------
    def each(self, fn):
        """fn(k, train_step) for k = 0 .. K - 1, each under member k's stream, between the fork and the join (module
        docstring); returns the list of fn's return values, their tensors marked for the caller's stream.  What has no method
        of its own goes through here: ens.each(lambda k, tr: tr.accumulate_series(A, parts[k], ...)), then
        ens.each(lambda k, tr: tr.apply())."""
        cur = _cuda.current_stream(self.device)
        before = [tr.steps for tr in self.members]
        used = range(min(self.K, self.n_streams))
        self._fork.record(cur)
        for s in used:
            self.side[s].wait_event(self._fork)
        out = [None] * self.K
        try:
            for k, tr in enumerate(self.members):
                _cuda.set_stream(self.side[k % self.n_streams])     # (torch.cuda.stream(...) without the context manager)
                out[k] = fn(k, tr)
        finally:                        # (also after a member that raised: what the others enqueued stays ordered)
            _cuda.set_stream(cur)
            for s in used:
                self._done[s].record(self.side[s])
                cur.wait_event(self._done[s])
        _hand_back(out, cur)
        self._check_after(before)
        return out

    def _fan(self, method, names, args, kwargs):
        per = self._resolve(method, names, args, kwargs)
        return self.each(lambda k, tr: getattr(tr, method)(*per[k][0], **per[k][1]))

    def step(self, A, X, L, **kw):
        """TrainStep.step of every member; returns the list of the members' (loss, Y).  `loss` is each member's own view,
        overwritten by its next step; ens.loss stacks them."""
        return self._fan("step", ("A", "X", "L"), (A, X, L), kw)

    def step_series(self, A, series, Ls, seq_len, **kw):
        """TrainStep.step_series of every member (stride / n_windows / starts, missing_labels, the loss spec and compact by
        keyword -- compact= goes through **kw to every member here and in forward_backward_series / validate_series, and each
        member compacts its own table: members on different folds of one series each run the front end on their fold's hours);
        the list of the members' (loss, Y)."""
        return self._fan("step_series", ("A", "series", "Ls", "seq_len"), (A, series, Ls, seq_len), kw)

    def forward_backward(self, A, X, L, **kw):
        return self._fan("forward_backward", ("A", "X", "L"), (A, X, L), kw)

    def forward_backward_series(self, A, series, Ls, seq_len, **kw):
        return self._fan("forward_backward_series", ("A", "series", "Ls", "seq_len"), (A, series, Ls, seq_len), kw)

    def validate(self, A, X, L, **kw):
        """TrainStep.validate of every member; the list of the members' val_loss views (ens.val_loss stacks them)."""
        return self._fan("validate", ("A", "X", "L"), (A, X, L), kw)

    def validate_series(self, A, series, Ls, seq_len, **kw):
        return self._fan("validate_series", ("A", "series", "Ls", "seq_len"), (A, series, Ls, seq_len), kw)

    def restore_best(self):
        """TrainStep.restore_best of every member (each reads its best_step on the host, as it does alone)."""
        return self._fan("restore_best", (), (), {})

    # ---- the range check ------------------------------------------------------------------------------------------------------
    def _check_after(self, before):
        ce = self.check_every
        if ce and any(tr.steps // ce > b // ce and tr.model.math != _lib.MATH_F32 for tr, b in zip(self.members, before)):
            self.check()

    def check(self):
        """The members' range check (TrainStep.check) after a join: the status word of every side stream's workspace -- a
        report names the members of that stream -- then of the process's other workspaces (one 4-byte read each)."""
        for s, stream in enumerate(self.side):
            buf = _F._Workspace._bufs.get((self.device.index, stream.cuda_stream))
            if buf is None:
                continue
            word = int(buf[:4].view(torch.int32).item())
            if word:
                buf[:4].zero_()
                what = "; ".join(t for b, t in _F._STATUS_TEXT.items() if word & b)
                raise RuntimeError("windgnn_amd: Ensemble: a kernel of member%s %s (side stream %d of %d) reported status %d: %s"
                                   % ("" if len(self.members_of(s)) == 1 else "s", ", ".join(map(str, self.members_of(s))), s,
                                      self.n_streams, word, what))
        _F.check_range_status(self.device)

    # ---- views ----------------------------------------------------------------------------------------------------------------
    def _stack(self, name):
        return torch.stack([getattr(tr, name) for tr in self.members])

    @property
    def loss(self):
        """[K]: the members' last losses, stacked on the caller's stream (a copy; no host read)."""
        return torch.stack([tr._loss for tr in self.members])

    val_loss = property(lambda self: self._stack("val_loss"), doc="[K] fp32: TrainStep.val_loss of every member")
    val_count = property(lambda self: self._stack("val_count"), doc="[K] int64: TrainStep.val_count of every member")
    val_stale = property(lambda self: self._stack("val_stale"), doc="[K] int64: TrainStep.val_stale of every member")
    best_loss = property(lambda self: self._stack("best_loss"), doc="[K] fp64: TrainStep.best_loss of every member")
    best_step = property(lambda self: self._stack("best_step"), doc="[K] int64: TrainStep.best_step of every member")

    @property
    def grad_norm(self):
        """[K] fp32: TrainStep.grad_norm of every member built with max_grad_norm (float('inf') measures), NaN for a member
        built with max_grad_norm=None.  With no measuring member at all it raises as TrainStep.grad_norm does."""
        if all(tr.max_grad_norm is None for tr in self.members):
            return self.members[0].grad_norm
        ref = next(tr.grad_norm for tr in self.members if tr.max_grad_norm is not None)
        nan = torch.full_like(ref, float("nan"))
        return torch.stack([tr.grad_norm if tr.max_grad_norm is not None else nan for tr in self.members])

    @property
    def steps(self):
        """[K] int64 on the device: the members' completed steps (host integers, uploaded without a synchronisation)."""
        return _upload(torch.tensor([tr.steps for tr in self.members], dtype=torch.int64), self.device)

    # ---- forecasts ------------------------------------------------------------------------------------------------------------
    def _forecast_models(self, who, use_best):
        if not use_best:
            return [tr.model for tr in self.members]
        for k, tr in enumerate(self.members):
            if tr._best_views is None:
                raise RuntimeError("windgnn_amd: Ensemble.%s(use_best=True): member %d was built with keep_best=None and keeps no "
                                   "snapshot" % (who, k))
        return [_BestOf(tr) for tr in self.members]

    def _forecast(self, n, H, run):
        # allocated on the caller's stream before the fork: the members copy their rows in under their own streams
        members = torch.empty(self.K, n, H, dtype=torch.float32, device=self.device)

        def member(k, tr):
            members[k].copy_(run(k))
        self.each(member)
        mean, std = mean_std(members)
        return EnsembleForecast(mean, std, members)

    def forward_last_series(self, adj, series, seq_len, wind_min, wind_max, stride=None, n_windows=None, starts=None,
                            use_best=False, compact=False):
        """The rolling backtest of every member (series.forward_last_series) as EnsembleForecast(mean, std, members):
        members [K, n, 3S] holds each member's de-normalised last rows, exactly what the member returns alone; mean and std
        [n, 3S] are mean_std's.  use_best=True: from each member's best snapshot (TrainStep(keep_best=...)) instead of its
        current parameters; a member that has kept nothing yet (best_step = -1) forecasts from a snapshot of zeros.  starts may
        be a PerMember of tables of one length.  compact: series.forward_last_series', passed to every member."""
        from .series import forward_last_series as one
        who = "forward_last_series"
        models = self._forecast_models(who, use_best)
        per = self._resolve(who, ("adj", "series"), (adj, series), dict(stride=stride, n_windows=n_windows, starts=starts,
                                                                      **({"compact": compact} if compact is not False else {})))
        counts = []
        for (a, kw) in per:
            if kw["starts"] is not None:
                counts.append(len(kw["starts"]))
            elif kw["n_windows"] is not None:
                counts.append(int(kw["n_windows"]))
            else:
                counts.append(n_series_windows(a[1].shape[0], int(seq_len), 1 if kw["stride"] is None else int(kw["stride"])))
        if len(set(counts)) != 1:
            raise ValueError("windgnn_amd: Ensemble.forward_last_series: the members forecast %s windows; mean and std need the "
                             "same windows of every member" % counts)
        H = self.members[0].p_views[5].shape[1]
        return self._forecast(counts[0], H, lambda k: one(models[k], per[k][0][0], per[k][0][1], seq_len, wind_min, wind_max,
                                                          **per[k][1]))

    def forward_last(self, adj, X, wind_min, wind_max, use_best=False):
        """data.forward_last of every member on the materialised windows X [B, T, S, 13] as EnsembleForecast(mean, std,
        members [K, B, 3S]); use_best as in forward_last_series."""
        from .data import forward_last as one
        models = self._forecast_models("forward_last", use_best)
        per = self._resolve("forward_last", ("adj", "X"), (adj, X), {})
        shapes = {tuple(a[1].shape[:1]) for a, _ in per}
        if len(shapes) != 1:
            raise ValueError("windgnn_amd: Ensemble.forward_last: the members forecast %s windows; mean and std need the same "
                             "windows of every member" % sorted(shapes))
        H = self.members[0].p_views[5].shape[1]
        return self._forecast(shapes.pop()[0], H, lambda k: one(models[k], per[k][0][0], per[k][0][1], wind_min, wind_max))

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """{"K": K, "members": [TrainStep.state_dict() of member 0 .. K - 1]}; the parameters travel through the models' own
        state_dict(), as with one TrainStep."""
        return {"K": self.K, "members": [tr.state_dict() for tr in self.members]}

    def load_state_dict(self, sd):
        if "K" not in sd or "members" not in sd or len(sd["members"]) != sd["K"]:
            raise ValueError("windgnn_amd: Ensemble.load_state_dict: expected {'K': K, 'members': [K TrainStep state dicts]}")
        if int(sd["K"]) != self.K:
            raise RuntimeError("windgnn_amd: Ensemble.load_state_dict: the checkpoint holds K = %d members, this ensemble %d"
                               % (int(sd["K"]), self.K))
        for tr, one in zip(self.members, sd["members"]):
            tr.load_state_dict(one)

    def workspace_bytes(self):
        """Bytes of the side streams' workspaces as they stand (functional._Workspace: one per stream, grow-only)."""
        total = 0
        for stream in self.side:
            buf = _F._Workspace._bufs.get((self.device.index, stream.cuda_stream))
            total += buf.numel() if buf is not None else 0
        return total


__all__ = ["Ensemble", "EnsembleForecast", "PerMember", "mean_std"]
