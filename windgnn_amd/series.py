"""Series mode (include/windgnn_series.h): the model on every sliding window of ONE hourly series, without building the
windows.

Window w = 0 .. n-1 covers rows w*stride .. w*stride + T - 1 of `series` [rows, S, 13] and starts from h = 0; the results are
those of GCN_GRU.forward on the materialised windows (make_windows(starts=...)).  What depends on the hour alone -- both graph
convolutions and the GRU's input projection -- runs once per hour instead of once per window and hour.

With `starts` (include/windgnn_series_at.h) the windows begin at a table of rows instead of w*stride: a series with outages
(segment_starts), a hold-out at window level, a shuffled mini-batch.  The front end then runs on every row of the series passed,
or with compact= (compact_table) on the rows some window covers alone.

Exact fp32 with a dense adjacency (S <= 64) and H <= 128 only; everything else raises and names the materialised path."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .functional import (_adj, _flat_grads, _params_struct, _ptr, _require_contiguous, _require_gpu, _stash_ptr, _stream,
                         _workspace)

_MATERIALISED = ("materialise the windows (windgnn_amd.data.make_windows(feat, seq_len, starts=...)) and call "
                 "GCN_GRU.forward / forward_last on them instead")


def n_series_windows(rows: int, seq_len: int, stride: int = 1) -> int:
    """Windows of seq_len rows, `stride` rows apart, that fit into a series of `rows` rows (0 if none does)."""
    if seq_len < 1 or stride < 1:
        raise ValueError("n_series_windows: seq_len and stride must be >= 1, got %d and %d" % (seq_len, stride))
    return 0 if rows < seq_len else (rows - seq_len) // stride + 1


def series_coverage(rows: int, seq_len: int, stride: int, n: int) -> List[Tuple[int, int]]:
    """Per series row tau the inclusive range (w_lo, w_hi) of the windows that cover it -- w*stride <= tau < w*stride +
    seq_len, 0 <= w < n -- in the closed form the fold kernel of the backward uses; w_lo > w_hi: no window covers the row
    (a gap when stride > seq_len, or a spare trailing row) and its gate gradient is zero.  Plain Python, no device."""
    if n < 1 or stride < 1 or seq_len < 1 or (n - 1) * stride + seq_len > rows:
        raise ValueError("series_coverage: %d windows of %d rows, %d apart, do not fit into %d rows" % (n, seq_len, stride, rows))
    out = []
    for tau in range(rows):
        w_hi = min(tau // stride, n - 1)
        w_lo = (tau - seq_len) // stride + 1 if tau >= seq_len else 0
        out.append((w_lo, w_hi))
    return out


def segment_starts(segments, seq_len: int, stride: int = 1, horizon: int = 0) -> List[int]:
    """The ascending starts of every window of seq_len rows that, together with `horizon` further label hours, lies inside ONE
    of `segments`, a list of (first_row, n_rows) clean stretches of a series: per segment first_row, first_row + stride, ...
    while start + seq_len + horizon <= first_row + n_rows.  A segment shorter than seq_len + horizon gives none; segments that
    overlap give the windows of each (duplicates included).  Plain Python, no device."""
    if seq_len < 1 or stride < 1 or horizon < 0:
        raise ValueError("segment_starts: seq_len and stride must be >= 1 and horizon >= 0, got %r, %r and %r"
                         % (seq_len, stride, horizon))
    out = []
    for first, count in segments:
        first, count = int(first), int(count)
        if first < 0 or count < 0:
            raise ValueError("segment_starts: a segment is (first_row >= 0, n_rows >= 0), got (%d, %d)" % (first, count))
        out.extend(range(first, first + count - seq_len - horizon + 1, stride))
    return sorted(out)


def starts_coverage(starts, seq_len: int, rows: int) -> np.ndarray:
    """[rows, 2] int64: per series row tau the half-open index range [lo, hi) of the windows of the NON-DECREASING table
    `starts` that cover it -- tau - seq_len < starts[w] <= tau -- as the fold kernel of the backward finds it (two binary
    searches); lo == hi: no window covers the row and its gate gradient is zero.  numpy, no device."""
    st = np.asarray(starts, dtype=np.int64).reshape(-1)
    if seq_len < 1 or rows < seq_len or (st.size and (np.any(np.diff(st) < 0) or st[0] < 0 or st[-1] > rows - seq_len)):
        raise ValueError("starts_coverage: starts must be non-decreasing within [0, rows - seq_len = %d]" % (rows - seq_len))
    tau = np.arange(rows, dtype=np.int64)
    return np.stack([np.searchsorted(st, tau - seq_len, side="right"), np.searchsorted(st, tau, side="right")], axis=1)


def kfold_starts(starts, k: int, seq_len: int, horizon: int = 3):
    """k folds of a table of window starts, blocked in time and purged: [(train, val)] * k, int64 numpy arrays.  The sorted
    table is cut into k blocks of consecutive entries (the first len % k one longer); block j is fold j's validation table.
    A window at row s reads rows [s, s + seq_len) and its labels reach `horizon` rows further, so its footprint is
    [s, s + seq_len + horizon).  Fold j's training table is every start of the other blocks whose footprint does not intersect
    the footprint of any window of block j: what a training window or its labels would share with a validation window or its
    labels is dropped (the windows next to a block's ends; a duplicate of a validation start).  Together with
    ens.step_series(..., starts=PerMember(trains)) and ens.validate_series(..., starts=PerMember(vals)) this is a blocked
    cross-validation with one Ensemble member per fold.  numpy, no device."""
    st = np.asarray(starts)
    if st.ndim != 1 or (st.size and st.dtype.kind not in "iu"):
        raise ValueError("kfold_starts: starts must be a 1-D sequence of integers, got dtype %s, shape %s" % (st.dtype, st.shape))
    if int(seq_len) < 1 or int(horizon) < 0:
        raise ValueError("kfold_starts: seq_len must be >= 1 and horizon >= 0, got %r and %r" % (seq_len, horizon))
    if int(k) != k or int(k) < 2:
        raise ValueError("kfold_starts: k=%r: at least two folds (one fold would validate on everything and train on nothing)" % (k,))
    if int(k) > st.size:
        raise ValueError("kfold_starts: k=%d folds of a table of %d starts: every fold needs a window to validate on" % (k, st.size))
    st = np.sort(st.astype(np.int64), kind="stable")
    span = int(seq_len) + int(horizon)
    out = []
    for val in np.array_split(st, int(k)):
        # footprints of one length intersect iff the starts are closer than it: the nearest validation start above s - span
        i = np.searchsorted(val, st - span, side="right")
        near = val[np.minimum(i, val.size - 1)]
        touches = (i < val.size) & (near < st + span)
        out.append((st[~touches], val.copy()))
    return out


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    """A host tensor on `device`, stream-ordered: from pinned memory, so the host does not wait for the work already queued on the
    current stream (a pageable upload would, and the calls that take a table promise not to synchronise)."""
    if torch.device(device).type == "cpu":
        return t
    return t.pin_memory().to(device, non_blocking=True)


def _starts_table(starts, rows: int, seq_len: int, device, who: str, ordered: bool):
    """`starts` as the int32 device table the _at entry points take.  A list / numpy array / CPU tensor is checked here, before
    the upload (integer dtype, one dimension, every entry in [0, rows - seq_len], and non-decreasing where `ordered`):
    ValueError.  A device tensor is taken as it is -- its values are checked by the kernel (WGNN_STATUS_WINDOW_START, raised
    by check_range_status) so that no call synchronises."""
    if rows < seq_len:
        raise RuntimeError("windgnn_amd: no window of %d rows fits into a series of %d rows" % (seq_len, rows))
    if isinstance(starts, torch.Tensor) and starts.device.type != "cpu":
        if starts.dtype not in (torch.int32, torch.int64) or starts.dim() != 1:
            raise ValueError("%s: starts must be a 1-D int32 / int64 tensor, got %s %s" % (who, starts.dtype, tuple(starts.shape)))
        if starts.device != device:
            raise ValueError("%s: starts is on %s, the series on %s" % (who, starts.device, device))
        return starts.to(torch.int32).contiguous()
    host = starts.numpy() if isinstance(starts, torch.Tensor) else np.asarray(starts)
    if host.size == 0:
        host = host.astype(np.int64)
    if host.dtype.kind not in "iu" or host.ndim != 1:
        raise ValueError("%s: starts must be a 1-D sequence of integers, got dtype %s, shape %s" % (who, host.dtype, host.shape))
    host = host.astype(np.int64)
    bad = np.nonzero((host < 0) | (host > rows - seq_len))[0]
    if bad.size:
        raise ValueError("%s: starts[%d] = %d, but a window of %d rows in a series of %d rows starts at 0 .. %d"
                         % (who, bad[0], host[bad[0]], seq_len, rows, rows - seq_len))
    if ordered and np.any(np.diff(host) < 0):
        w = int(np.nonzero(np.diff(host) < 0)[0][0]) + 1
        raise ValueError("%s: starts must be non-decreasing here, but starts[%d] = %d < starts[%d] = %d (GCN_GRU.forward_series "
                         "and TrainStep.step_series take any order)" % (who, w, host[w], w - 1, host[w - 1]))
    return _upload(torch.from_numpy(host.astype(np.int32)), device)


def sorted_starts(starts, rows: int, seq_len: int, device, who: str):
    """(table, inverse): `starts` in any order as the sorted int32 device table, and the index tensor that takes rows of the
    sorted call's Y back into the caller's order (None: the order was the caller's already).  A host table is sorted on the host;
    a device table on the device, without a synchronisation."""
    if isinstance(starts, torch.Tensor) and starts.device.type != "cpu":
        table = _starts_table(starts, rows, seq_len, device, who, ordered=False)
        table, order = torch.sort(table, stable=True)
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(order.numel(), device=device)
        return table, inverse
    table = _starts_table(starts, rows, seq_len, "cpu", who, ordered=False)
    table, order = torch.sort(table, stable=True)
    if torch.equal(order, torch.arange(order.numel())):
        return _upload(table, device), None
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel())
    return _upload(table, device), _upload(inverse, device)


# ---- covered hours only ------------------------------------------------------------------------------------------------------
# compact="auto" compacts when the compacted series has at most this share of the rows, as measured on step_series at the
# reference's widths (profiles/r22_series_compact_cost.txt, DESIGN.md section 5, "Covered hours only"): a host table up to 0.37; a
# device table never (the dozen small launches of the device-side compaction cost a step more than the shorter front end
# saves), and neither do the forward-only calls (validate_series, forward_last_series)
COMPACT_AUTO_THETA = 0.37
COMPACT_AUTO_THETA_DEVICE = 0.0


class CompactTable(NamedTuple):
    """compact_table's record.  hours [rows_c] int64: the series row behind every row of the compacted series; table [n] int32:
    the windows' starts in the compacted series; rows_c: its row count (a host int); covered: m, the number of hours any window
    covers (a host int for a host table, a 0-dim device tensor for a device table)."""
    hours: torch.Tensor
    table: torch.Tensor
    rows_c: int
    covered: object

    def apply(self, series: torch.Tensor, Ls: torch.Tensor):
        """(series_c, Ls_c): the rows `hours` of the series and of the label series (NaN labels travel unchanged)."""
        return series.index_select(0, self.hours), Ls.index_select(0, self.hours)


def _is_device_table(starts) -> bool:
    return isinstance(starts, torch.Tensor) and starts.device.type != "cpu"


def compact_table(starts, rows: int, seq_len: int, cover_bound=None, device=None) -> CompactTable:
    """The windows of a NON-DECREASING table as windows of the series' COVERED hours alone.  C = the ascending hours
    U_w [starts[w], starts[w] + seq_len), m = |C|: hours[c] = C[c], table[w] = the rank of starts[w] in C, so that
    hours[table[w] + t] == starts[w] + t -- a window covers seq_len consecutive hours, hence seq_len consecutive ranks -- and
    a series call on (series[hours], Ls[hours], table) is the call on (series, Ls, starts) with a front end of rows_c rows.
    starts: what sorted_starts returns, checked as _starts_table checks it.
    A host table (list, numpy, CPU tensor): numpy on the host, rows_c = m exactly; the results are uploaded to `device` (None:
    they stay on the host) from pinned memory, as sorted_starts uploads.
    A device table: torch operations on the current stream with no host read and no data-dependent shape, so rows_c is the
    bound min(rows, n * seq_len) -- or min(rows, cover_bound), the caller's promise that the table covers at most that many
    hours -- and the rows m .. rows_c - 1, which no window covers, repeat hour C[0] (real, finite data).  A start outside
    [0, rows - seq_len] is clamped before it indexes anything and its window gets the entry -1, as does a window whose ranks
    do not fit under cover_bound: the table entry points then report WGNN_STATUS_WINDOW_START, as for any bad device table.
    device="cpu" with a host table runs that same arithmetic on CPU tensors."""
    rows, T = int(rows), int(seq_len)
    if T < 1 or rows < T:
        raise ValueError("compact_table: no window of %d rows fits into a series of %d rows" % (T, rows))
    if cover_bound is not None and (isinstance(cover_bound, bool) or int(cover_bound) != cover_bound or int(cover_bound) < T):
        raise ValueError("compact_table: cover_bound=%r must be an integer >= seq_len = %d, the hours one window covers"
                         % (cover_bound, T))
    on_device = _is_device_table(starts)
    if on_device and device is not None and torch.device(device) != starts.device:
        raise ValueError("compact_table: starts is on %s, device= says %s" % (starts.device, device))
    if not on_device and (device is None or torch.device(device).type != "cpu"):
        st = _starts_table(starts, rows, T, "cpu", "compact_table", ordered=True).numpy().astype(np.int64)
        if st.size < 1:
            raise ValueError("compact_table: the table of starts is empty")
        diff = np.zeros(rows + 1, dtype=np.int64)
        np.add.at(diff, st, 1)
        np.add.at(diff, st + T, -1)
        cov = np.cumsum(diff[:rows]) > 0
        hours = np.flatnonzero(cov)
        m = int(hours.size)
        if cover_bound is not None and m > int(cover_bound):
            raise ValueError("compact_table: the table covers %d hours, more than cover_bound=%d" % (m, int(cover_bound)))
        table = (np.cumsum(cov) - cov)[st].astype(np.int32)
        to = "cpu" if device is None else device
        return CompactTable(_upload(torch.from_numpy(hours), to), _upload(torch.from_numpy(table), to), m, m)
    if not isinstance(starts, torch.Tensor):
        starts = _starts_table(starts, rows, T, "cpu", "compact_table", ordered=True)
    if starts.dtype not in (torch.int32, torch.int64) or starts.dim() != 1 or starts.numel() < 1:
        raise ValueError("compact_table: starts must be a 1-D int32 / int64 tensor of at least one entry, got %s %s"
                         % (starts.dtype, tuple(starts.shape)))
    dev, n = starts.device, starts.numel()
    rows_c = min(rows, n * T if cover_bound is None else int(cover_bound))
    s = starts.to(torch.int64)
    ok = (s >= 0) & (s <= rows - T)
    s = s.clamp(0, rows - T)                            # from here on every index is in range, whatever the table held
    one = ok.to(torch.int64)
    diff = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    diff.index_add_(0, s, one)                          # (integer adds: any order gives the same sums)
    diff.index_add_(0, s + T, -one)
    cov = (diff[:rows].cumsum(0) > 0).to(torch.int64)
    incl = cov.cumsum(0)
    rank, m = incl - cov, incl[rows - 1]
    tau = torch.arange(rows, dtype=torch.int64, device=dev)
    slot = torch.where((cov > 0) & (rank < rows_c), rank, torch.full_like(rank, rows_c))      # rows_c: the dump slot
    hours = torch.zeros(rows_c + 1, dtype=torch.int64, device=dev).scatter_(0, slot, tau)[:rows_c]
    c = torch.arange(rows_c, dtype=torch.int64, device=dev)
    hours = torch.where(c < m, hours, hours[0])         # (m = 0: every window was bad, and hour 0 is as real as any)
    t = rank.index_select(0, s)
    table = torch.where(ok & (t + T <= rows_c), t, torch.full_like(t, -1)).to(torch.int32)
    return CompactTable(hours, table, rows_c, m)


def _compact_arg(who: str, compact, starts, stride=None):
    """compact= of a series call as (wanted, auto, cover_bound); refused by name before any launch where it makes no sense."""
    if compact is False or compact is None:
        return False, False, None
    if not (compact is True or compact == "auto" or (isinstance(compact, int) and not isinstance(compact, bool))):
        raise ValueError("%s: compact=%r: False, True, 'auto', or an int, the number of hours the table covers at most"
                         % (who, compact))
    if starts is None or stride not in (None, 0):
        raise ValueError("%s: compact=%r belongs to starts=: the strided windows cover the series densely, so there is no hour to "
                         "drop (got %s)" % (who, compact, "stride=%r" % (stride,) if stride not in (None, 0) else "no table of starts"))
    if isinstance(compact, int) and not isinstance(compact, bool):
        return True, False, int(compact)
    return True, compact == "auto", None


def compacted_starts(starts, series, Ls, seq_len: int, who: str, compact, forward_only=False):
    """sorted_starts for a call that takes compact=: (series, Ls, table, inverse) -- the series and the label series the raw
    calls get (Ls may be None), the sorted int32 device table into them, and sorted_starts' inverse permutation.  With
    compact=False, with a table that leaves no row to drop (rows_c == rows) and with "auto" above COMPACT_AUTO_THETA (a host
    table; COMPACT_AUTO_THETA_DEVICE for a device table; never for a forward_only call) these are the series as it is and
    sorted_starts' own results; otherwise compact_table's, the host table compacted on the host and uploaded once.  Ls must
    have been checked to hold a row per series row."""
    want, auto, bound = _compact_arg(who, compact, starts)
    rows, T, device = series.shape[0], int(seq_len), series.device
    if not want:
        return (series, Ls, *sorted_starts(starts, rows, T, device, who))
    if bound is not None and bound < T:
        raise ValueError("%s: compact=%d: a table covers at least the seq_len = %d hours of one window" % (who, bound, T))
    on_device = _is_device_table(starts)
    table, inverse = sorted_starts(starts, rows, T, device if on_device else "cpu", who)
    theta = 0.0 if forward_only else (COMPACT_AUTO_THETA_DEVICE if on_device else COMPACT_AUTO_THETA)
    pays = lambda rows_c: rows_c < rows and not (auto and rows_c > theta * rows)   # noqa: E731
    ct = None
    if table.numel() >= 1 and on_device:
        if pays(min(rows, table.numel() * T if bound is None else bound)):
            ct = compact_table(table, rows, T, bound)
    elif table.numel() >= 1:
        ct = compact_table(table, rows, T, bound)
        ct = ct if pays(ct.rows_c) else None
    if not on_device:       # one upload each, after the decision: the sorted table or the compacted one, never both
        table, inverse = (_upload(table, device) if ct is None else None), (None if inverse is None else _upload(inverse, device))
        ct = ct and CompactTable(_upload(ct.hours, device), _upload(ct.table, device), ct.rows_c, ct.covered)
    if ct is None:
        return series, Ls, table, inverse
    return series.index_select(0, ct.hours), (None if Ls is None else Ls.index_select(0, ct.hours)), ct.table, inverse


def _no_stride_with_starts(who: str, stride, starts, n_windows=None) -> None:
    if starts is not None and stride not in (None, 0):
        raise ValueError("%s: pass stride= or starts=, not both (got stride=%r with a table of starts)" % (who, stride))
    if starts is not None and n_windows is not None:
        raise ValueError("%s: n_windows= belongs to stride=; with starts= the table's length is the window count" % who)


def _fn(lib, name: str, sd):
    """The entry point `name` of the family sd belongs to: wgnn_series_<name>, or its _at form for a table (stride = 0)."""
    if sd.stride != 0:
        return getattr(lib, "wgnn_series_" + name)
    return getattr(lib, ("wgnn_series_at_%s" if name.endswith("_bytes") else "wgnn_series_%s_at") % name)


def _series_setup(A, series, seq_len: int, stride: int, params: Sequence[torch.Tensor], math: int, n_windows=None, starts=None,
                  ws_query=None):
    """Everything a series call checks and sizes before it launches: (adjacency, dims, workspace, workspace bytes); with
    `starts` also the int32 device table (dims.stride = 0, dims.n = its length), as a fifth result.  ws_query: the size query
    of an entry point with a workspace of its own (series_val_raw)."""
    if hasattr(A, "blob"):
        raise RuntimeError("windgnn_amd: series mode takes a dense adjacency (S <= 64), not a CsrAdjacency: " + _MATERIALISED)
    if math != _lib.MATH_F32:
        raise RuntimeError("windgnn_amd: series mode runs in exact fp32 (math='f32') only, not in the fp16-plane modes "
                           "(f16x3 / f16x3g / f16): " + _MATERIALISED)
    _require_gpu(series)
    _require_gpu(*params)
    _require_contiguous(series=series, params=params)
    if series.dim() != 3:
        raise RuntimeError("windgnn_amd: series must be [rows, S, 13], got %s" % (tuple(series.shape),))
    rows, S, F = series.shape
    if starts is not None:
        _no_stride_with_starts("windgnn_amd series mode", stride, starts, n_windows)
        table = _starts_table(starts, rows, seq_len, series.device, "windgnn_amd series mode", ordered=True)
        if table.numel() < 1:
            raise RuntimeError("windgnn_amd: the table of starts is empty: a series call needs at least one window")
        A, fmt, nnz = _adj(A, S)
        H = params[5].shape[1]
        sd = _lib.SeriesDims(rows, seq_len, 0, table.numel(), S, F, H, math, fmt, nnz, _lib.IO_F32)
        ws, ws_bytes = _workspace(sd, series.device,
                                  refused="wgnn_series_at_workspace_bytes(rows=%d,T=%d,n=%d,S=%d,F=%d,H=%d) [%s]"
                                  % (rows, seq_len, table.numel(), S, F, H, _MATERIALISED), query=ws_query)
        return A, sd, ws, ws_bytes, table
    fit = n_series_windows(rows, seq_len, stride)
    if fit < 1:
        raise RuntimeError("windgnn_amd: no window of %d rows fits into a series of %d rows" % (seq_len, rows))
    n = fit if n_windows is None else int(n_windows)
    if n < 1 or n > fit:
        raise RuntimeError("windgnn_amd: n_windows = %d, but a series of %d rows holds 1 .. %d windows of %d rows at stride %d"
                           % (n, rows, fit, seq_len, stride))
    A, fmt, nnz = _adj(A, S)
    H = params[5].shape[1]
    sd = _lib.SeriesDims(rows, seq_len, stride, n, S, F, H, math, fmt, nnz, _lib.IO_F32)
    ws, ws_bytes = _workspace(sd, series.device,
                              refused="wgnn_series_workspace_bytes(rows=%d,T=%d,stride=%d,n=%d,S=%d,F=%d,H=%d) [%s]"
                              % (rows, seq_len, stride, n, S, F, H, _MATERIALISED), query=ws_query)
    return A, sd, ws, ws_bytes


def _table_arg(sd, starts=None):
    """The `starts` argument of an _at entry point as a tuple to splice in after Xs (empty for the strided family)."""
    if sd.stride != 0:
        if starts is not None:
            raise ValueError("windgnn_amd: these dims have stride %d: they take no table of starts" % sd.stride)
        return ()
    if (starts is None or starts.dtype != torch.int32 or starts.dim() != 1 or starts.numel() != sd.n
            or not starts.is_contiguous()):
        raise ValueError("windgnn_amd: dims with stride = 0 take starts=, the contiguous int32 device table of n = %d entries "
                         "the forward was given" % sd.n)
    if not starts.is_cuda:
        raise RuntimeError("windgnn_amd runs on an MI355X (HIP) only: the table of starts is a %s tensor" % starts.device)
    return (_ptr(starts),)


def series_forward_raw(A, series, seq_len, stride, params, math=_lib.MATH_F32, want_stash=True, n_windows=None, starts=None):
    """Y [n, T, H], stash, dims = wgnn_series_fwd(...).  n_windows: the first that many windows (default: all that fit).
    starts (with stride None): a NON-DECREASING table of window starts -- wgnn_series_fwd_at; a fourth result is then the int32
    device table to hand to series_backward_raw."""
    lib = _lib.load()
    A, sd, ws, ws_bytes, *table = _series_setup(A, series, seq_len, stride, params, math, n_windows, starts)
    stash = (torch.empty(_fn(lib, "stash_bytes", sd)(C.byref(sd)), dtype=torch.uint8, device=series.device)
             if want_stash else None)
    Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params)
    at = _table_arg(sd, *table)
    rc = _fn(lib, "fwd", sd)(C.byref(sd), _ptr(A), _ptr(series), *at, C.byref(ps), _ptr(Y), _stash_ptr(stash), _ptr(ws),
                             ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_fwd_at" if at else "wgnn_series_fwd")
    return (Y, stash, sd, *table)


def series_backward_raw(sd, A, series, params, Y, dY, stash, grads: Sequence[torch.Tensor], starts=None) -> None:
    """wgnn_series_bwd: the 8 gradients of sum(Y * dY), summed over all windows, into `grads` (overwritten).  starts: the
    forward's table (dims with stride = 0: wgnn_series_bwd_at)."""
    lib = _lib.load()
    _require_contiguous(series=series, Y=Y, dY=dY, adj_matrix=A, grads=grads, params=params)
    at = _table_arg(sd, starts)
    ws, ws_bytes = _workspace(sd, series.device)
    ps = _params_struct(_lib.Params, params)
    gs = _params_struct(_lib.Grads, grads)
    rc = _fn(lib, "bwd", sd)(C.byref(sd), _ptr(A), _ptr(series), *at, C.byref(ps), _ptr(Y), _ptr(dY), _stash_ptr(stash),
                             C.byref(gs), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_bwd_at" if at else "wgnn_series_bwd")


def _check_label_series(Ls, sd) -> None:
    """Ls as series_labels returns it: contiguous [rows, H] fp32 on the GPU with a row for every hour a window covers."""
    if sd.stride == 0 and (Ls.dim() != 2 or Ls.shape[1] != sd.H or Ls.shape[0] < sd.rows):
        raise RuntimeError("windgnn_amd: with a table of starts the label series Ls must be [rows >= the series' %d, H = %d] (a "
                           "window may start at any row up to rows - seq_len), got %s" % (sd.rows, sd.H, tuple(Ls.shape)))
    need = (sd.n - 1) * sd.stride + sd.T
    if Ls.dim() != 2 or Ls.shape[1] != sd.H or Ls.shape[0] < need:
        raise RuntimeError("windgnn_amd: the label series Ls must be [rows >= (n - 1) * stride + seq_len = %d, H = %d] (what "
                           "series_labels(feat, seq_len, stride, n_windows)[0] returns; its window view L is not needed), got %s"
                           % (need, sd.H, tuple(Ls.shape)))
    _require_gpu(Ls)
    _require_contiguous(Ls=Ls)


def _masked_table(at):
    """The `starts` argument of a masked entry point (include/windgnn_series_masked.h): one pair serves both row mappings, so
    the strided form passes NULL where the table goes."""
    return at if at else (None,)


def loss_spec(loss, huber_delta, loss_from, seq_len, missing_labels=False, who="windgnn_amd series mode"):
    """The wgnn_lossfn of loss= / huber_delta= / loss_from= (include/windgnn_series_lossfn.h), or None for the defaults ("mse"
    from step 0), which are the entry points that need no spec.  Everything the library would refuse is refused here first, by
    the argument's name."""
    import math as _math
    if loss not in _lib.LOSS_KINDS:
        raise ValueError("%s: loss=%r: the series recurrences form 'mse', 'l1' or 'huber'; any other loss works on "
                         "GCN_GRU.forward_series' output through autograd" % (who, loss))
    t_from = int(loss_from)
    if t_from != loss_from or not 0 <= t_from < int(seq_len):
        raise ValueError("%s: loss_from=%r must be a step of the window, an integer in [0, seq_len = %d): 0 counts every step, "
                         "seq_len - 1 the last alone" % (who, loss_from, int(seq_len)))
    delta = float(huber_delta)
    if loss == "huber" and not (_math.isfinite(delta) and delta > 0.0):
        raise ValueError("%s: huber_delta=%r must be finite and > 0 (nn.HuberLoss's delta); loss='l1' is the limit of a small "
                         "one and loss='mse' twice that of a large one" % (who, huber_delta))
    if loss == "mse" and t_from == 0:
        return None
    return _lib.LossFn(_lib.LOSS_KINDS[loss], delta if loss == "huber" else 0.0, t_from, 1 if missing_labels else 0)


def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=_lib.MATH_F32, n_windows=None, prepared=None,
                            starts=None, missing_labels=False, loss="mse", huber_delta=1.0, loss_from=0):
    """Y [n, T, H], stash, loss_buf, dims = wgnn_series_fwd_loss(...): series_forward_raw with the MSE statistics of (Y - labels)
    left in loss_buf for series_backward_mse_raw.  Ls [rows - 3, H]: the label SERIES (series_labels' first result); window w,
    step t reads its row w * stride + t.  starts (with stride None): a NON-DECREASING table, the row is starts[w] + t, Ls needs
    the series' rows, and a fifth result is the int32 device table (wgnn_series_fwd_loss_at).
    missing_labels=True (wgnn_series_fwd_loss_masked, either row mapping): a NaN in Ls is "no label" and enters neither the sum nor
    the count; loss_buf then has wgnn_series_masked_loss_bytes and goes to series_backward_mse_raw(..., missing_labels=True).
    loss="mse" | "l1" | "huber" (with huber_delta), loss_from=t: the statistics of that loss over the steps t .. seq_len - 1 of
    every window (wgnn_series_fwd_lossfn, either row mapping, with or without missing_labels); the backward takes the same
    keywords.  The defaults are the calls above."""
    lib = _lib.load()
    spec = loss_spec(loss, huber_delta, loss_from, seq_len, missing_labels)
    A, sd, ws, ws_bytes, *table = _series_setup(A, series, seq_len, stride, params, math, n_windows, starts)
    _check_label_series(Ls, sd)
    stash = torch.empty(_fn(lib, "stash_bytes", sd)(C.byref(sd)), dtype=torch.uint8, device=series.device)
    if spec is not None:
        loss_buf = torch.empty(lib.wgnn_series_lossfn_bytes(C.byref(sd)) // 4, dtype=torch.float32, device=series.device)
        Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
        ps = _params_struct(_lib.Params, params, prepared)
        rc = lib.wgnn_series_fwd_lossfn(C.byref(sd), _ptr(A), _ptr(series), *_masked_table(_table_arg(sd, *table)), C.byref(ps),
                                        _ptr(Ls), Ls.shape[0], C.byref(spec), _ptr(Y), _stash_ptr(stash), _ptr(loss_buf),
                                        _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "wgnn_series_fwd_lossfn")
        return (Y, stash, loss_buf, sd, *table)
    if missing_labels:
        loss_buf = torch.empty(lib.wgnn_series_masked_loss_bytes(C.byref(sd)) // 4, dtype=torch.float32, device=series.device)
        Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
        ps = _params_struct(_lib.Params, params, prepared)
        rc = lib.wgnn_series_fwd_loss_masked(C.byref(sd), _ptr(A), _ptr(series), *_masked_table(_table_arg(sd, *table)),
                                             C.byref(ps), _ptr(Ls), Ls.shape[0], _ptr(Y), _stash_ptr(stash), _ptr(loss_buf),
                                             _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "wgnn_series_fwd_loss_masked")
        return (Y, stash, loss_buf, sd, *table)
    loss_buf = torch.empty(_fn(lib, "loss_bytes", sd)(C.byref(sd)) // 4, dtype=torch.float32, device=series.device)
    Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params, prepared)
    at = _table_arg(sd, *table)
    rc = _fn(lib, "fwd_loss", sd)(C.byref(sd), _ptr(A), _ptr(series), *at, C.byref(ps), _ptr(Ls), Ls.shape[0], _ptr(Y),
                                  _stash_ptr(stash), _ptr(loss_buf), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_fwd_loss_at" if at else "wgnn_series_fwd_loss")
    return (Y, stash, loss_buf, sd, *table)


def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads: Sequence[torch.Tensor], loss: torch.Tensor,
                            grad_scale: float = 1.0, prepared=None, starts=None, missing_labels=False, loss_kind="mse",
                            huber_delta=1.0, loss_from=0) -> None:
    """wgnn_series_bwd_mse: the 8 gradients of grad_scale * mean((Y - labels)^2) into `grads` (overwritten, final) and the
    unweighted mean into `loss` (a 0-dim fp32 device tensor), without a dY tensor.  Y, stash, loss_buf: as
    series_forward_loss_raw returned them for the same inputs (starts: its table, for dims with stride = 0).
    missing_labels=True (wgnn_series_bwd_mse_masked; the forward's flag): the mean and the gradients are over the labels that are
    not NaN; with none at all the loss is NaN and the gradients are zero.
    loss_kind (the forward's loss=; `loss` is the output tensor here), huber_delta, loss_from: the forward's (wgnn_series_bwd_lossfn): the gradients of grad_scale * that loss over the steps
    loss_from .. seq_len - 1 and its unweighted value; other values than the forward's give a NaN loss and zero gradients."""
    lib = _lib.load()
    spec = loss_spec(loss_kind, huber_delta, loss_from, sd.T, missing_labels)
    _check_label_series(Ls, sd)
    _require_gpu(loss, loss_buf)
    _require_contiguous(series=series, Y=Y, adj_matrix=A, loss_buf=loss_buf, grads=grads, params=params)
    at = _table_arg(sd, starts)
    counted = missing_labels or spec is not None
    need = (lib.wgnn_series_masked_loss_bytes if counted else _fn(lib, "loss_bytes", sd))(C.byref(sd))
    if loss_buf.numel() * 4 < need:
        raise RuntimeError("windgnn_amd: loss_buf holds %d bytes, wgnn_series_%sloss_bytes says %d"
                           % (loss_buf.numel() * 4, "masked_" if counted else "", need))
    ws, ws_bytes = _workspace(sd, series.device)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    if spec is not None:
        rc = lib.wgnn_series_bwd_lossfn(C.byref(sd), _ptr(A), _ptr(series), *_masked_table(at), C.byref(ps), _ptr(Y), _ptr(Ls),
                                        Ls.shape[0], float(grad_scale), C.byref(spec), _stash_ptr(stash), _ptr(loss_buf),
                                        _ptr(loss), C.byref(gs), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "wgnn_series_bwd_lossfn")
        return
    if missing_labels:
        rc = lib.wgnn_series_bwd_mse_masked(C.byref(sd), _ptr(A), _ptr(series), *_masked_table(at), C.byref(ps), _ptr(Y),
                                            _ptr(Ls), Ls.shape[0], float(grad_scale), _stash_ptr(stash), _ptr(loss_buf),
                                            _ptr(loss), C.byref(gs), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "wgnn_series_bwd_mse_masked")
        return
    rc = _fn(lib, "bwd_mse", sd)(C.byref(sd), _ptr(A), _ptr(series), *at, C.byref(ps), _ptr(Y), _ptr(Ls), Ls.shape[0],
                                 float(grad_scale), _stash_ptr(stash), _ptr(loss_buf), _ptr(loss), C.byref(gs), _ptr(ws),
                                 ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_bwd_mse_at" if at else "wgnn_series_bwd_mse")


def val_spec(loss, huber_delta, loss_from, seq_len, missing_labels=False, who="windgnn_amd series mode"):
    """The wgnn_lossfn of a validation pass: loss_spec's checks and refusals, but always a spec -- wgnn_series_val has no entry
    point without one, so the defaults are {MSE, 0, step 0, masked}."""
    spec = loss_spec(loss, huber_delta, loss_from, seq_len, missing_labels, who)
    return spec if spec is not None else _lib.LossFn(_lib.LOSS_MSE, 0.0, 0, 1 if missing_labels else 0)


def series_val_raw(A, series, params, Ls, seq_len, stride=None, n_windows=None, math=_lib.MATH_F32, prepared=None, loss="mse",
                   huber_delta=1.0, loss_from=0, missing_labels=False, starts=None, last=None, out_loss=None, val=None,
                   wind_min=0.0, wind_max=1.0):
    """wgnn_series_val (include/windgnn_series_val.h): the loss of the spec loss= / huber_delta= / loss_from= / missing_labels= on
    the windows of `series` (stride / n_windows, or a NON-DECREASING table starts=), forward-only: no Y, no stash, no backward.
    last [n, H] (optional): Y[:, -1] * (wind_max - wind_min) + wind_min, as forward_last_series gives it; out_loss (a 0-dim or
    1-element fp32 device tensor, optional): the bits series_forward_loss_raw + series_backward_mse_raw would leave in their
    loss; val (functional.val_buffer, optional): the record this call's sums are added to.  At least one of out_loss / val.
    Returns (dims, table or None)."""
    from .functional import _val_ptr
    lib = _lib.load()
    spec = val_spec(loss, huber_delta, loss_from, seq_len, missing_labels)
    if out_loss is None and val is None:
        raise ValueError("windgnn_amd: series_val_raw needs out_loss= or val= (or both): there is nothing else to report the loss in")
    stride = None if starts is not None else (1 if stride is None else int(stride))
    A, sd, ws, ws_bytes, *table = _series_setup(A, series, seq_len, stride, params, math, n_windows, starts,
                                                ws_query="wgnn_series_val_workspace_bytes")
    _check_label_series(Ls, sd)
    if last is not None:
        _require_gpu(last)
        _require_contiguous(last=last)
        if tuple(last.shape) != (sd.n, sd.H):
            raise RuntimeError("windgnn_amd: series_val_raw: last must be [n = %d, H = %d], got %s" % (sd.n, sd.H, tuple(last.shape)))
    if out_loss is not None:
        _require_gpu(out_loss)
        if out_loss.numel() != 1:
            raise RuntimeError("windgnn_amd: series_val_raw: out_loss must hold one float, got %s" % (tuple(out_loss.shape),))
    ps = _params_struct(_lib.Params, params, prepared)
    rc = lib.wgnn_series_val(C.byref(sd), _ptr(A), _ptr(series), *_masked_table(_table_arg(sd, *table)), C.byref(ps), _ptr(Ls),
                             Ls.shape[0], C.byref(spec), float(wind_min), float(wind_max), _ptr(last), _ptr(out_loss),
                             _val_ptr(val) if val is not None else C.c_void_p(0), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_val")
    return sd, (table[0] if table else None)


class SeriesFunction(torch.autograd.Function):
    """Y [n, T, H] = GCN_GRU on every window of the series.  Gradients flow to the 8 parameters only, as in GCNGRUFunction."""

    @staticmethod
    def forward(ctx, A, series, seq_len, stride, n_windows, starts, math, *params):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[0]:
            raise RuntimeError("windgnn_amd: series mode gives gradients for the 8 parameters only; a series / adj_matrix "
                               "with requires_grad=True is not supported (detach it)")
        series = series.contiguous()
        params = tuple(p.contiguous() for p in params)
        need = any(ctx.needs_input_grad[7:])
        Y, stash, sd, *table = series_forward_raw(A, series, seq_len, stride, params, math, want_stash=need, n_windows=n_windows,
                                                  starts=starts)
        ctx.sd = sd
        ctx.table = table[0] if table else None      # (not a saved tensor: an index table, no gradient, never modified)
        ctx.save_for_backward(_adj(A)[0], series, Y, stash, *params)
        return Y

    @staticmethod
    def backward(ctx, dY):
        A, series, Y, stash, *params = ctx.saved_tensors
        if stash is None:
            raise RuntimeError("windgnn_amd: backward called but the forward ran without a stash")
        grads = _flat_grads(params, series.device)
        series_backward_raw(ctx.sd, A, series, params, Y, dY.float().contiguous(), stash, grads, starts=ctx.table)
        return (None, None, None, None, None, None, None, *grads)


def gcn_gru_series(A, series, seq_len: int, stride, params, math=_lib.MATH_F32, n_windows=None, starts=None):
    """Y [n, seq_len, H] for the first n = n_windows (default: all n_series_windows(rows, seq_len, stride)) windows of series
    [rows, S, 13]; or, with stride None and `starts` (NON-DECREASING; GCN_GRU.forward_series sorts), for the windows at those
    rows."""
    _no_stride_with_starts("gcn_gru_series", stride, starts, n_windows)
    return SeriesFunction.apply(A, series, int(seq_len), None if starts is not None else int(stride), n_windows, starts, math,
                                *params)


def _require_fused(model, who: str) -> None:
    if not getattr(model, "fused", False):
        raise RuntimeError("%s: series mode is built for the reference model's 13 / 13 widths only (got input_dim / "
                           "hidden_dim = %d / %d): %s" % (who, model.conv1.weight.shape[0], model.conv1.weight.shape[1],
                                                          _MATERIALISED))


def forward_last_series(model, adj_matrix, series: torch.Tensor, seq_len: int, wind_min: float, wind_max: float,
                        stride: int = None, n_windows=None, starts=None, compact=False) -> torch.Tensor:
    """The rolling backtest: [n, 3S] de-normalised forecasts, one per window, each from its own zero-state seq_len-hour
    window (wgnn_series_fwd_last; no Y is written).  The rows are what forward_last gives on the materialised windows and feed
    evaluate.eval_accum as they are.  stride defaults to 1.  starts (instead of stride / n_windows): the windows at that table
    of rows, in any order; row i of the result belongs to starts[i].  compact (with starts= only): the front end on the covered
    hours alone, as in TrainStep.step_series."""
    lib = _lib.load()
    _require_fused(model, "forward_last_series")
    _no_stride_with_starts("forward_last_series", stride, starts, n_windows)
    _compact_arg("forward_last_series", compact, starts, stride)
    params = [p.detach().contiguous() for p in model.hot_path_parameters()]
    series = series.contiguous()
    inverse = None
    if starts is not None:
        if series.dim() != 3:
            raise RuntimeError("windgnn_amd: series must be [rows, S, 13], got %s" % (tuple(series.shape),))
        series, _, starts, inverse = compacted_starts(starts, series, None, int(seq_len), "forward_last_series", compact,
                                                      forward_only=True)
    A, sd, ws, ws_bytes, *table = _series_setup(adj_matrix, series, int(seq_len), None if starts is not None else
                                                int(1 if stride is None else stride), params, model.math, n_windows, starts)
    out = torch.empty(sd.n, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params)
    at = _table_arg(sd, *table)
    rc = _fn(lib, "fwd_last", sd)(C.byref(sd), _ptr(A), _ptr(series), *at, C.byref(ps), float(wind_min), float(wind_max),
                                  _ptr(out), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_fwd_last_at" if at else "wgnn_series_fwd_last")
    return out if inverse is None else out.index_select(0, inverse)


def series_labels(feat: torch.Tensor, seq_len: int, stride: int = 1, n_windows: int = None):
    """(Ls, L): the labels of series mode.  A label row depends on the hour alone, Ls[tau] = [y[tau+1] | y[tau+2] | y[tau+3]]
    with y = feat[:, :, LABEL_FEATURE] (src/step4_sequence_preparer.py:14-19), so Ls [rows - 3, 3S] is built once and
    L [n, seq_len, 3S] is a VIEW of it (unfold: no copy), window-major like forward_series's output.  n = n_windows, or every
    window of seq_len rows that fits into feat (make_windows' count at stride = seq_len).  Works on any device.
    Raises where the last window's +3 h label does not fit into feat -- e.g. train on forward_series(adj, feat[:-3], ...) with
    series_labels(feat, ..., n_windows=n_series_windows(len(feat) - 3, seq_len, stride))."""
    from .data import LABEL_FEATURE
    if feat.dim() != 3:
        raise RuntimeError("windgnn_amd.series_labels: feat must be [rows, S, 13], got %s" % (tuple(feat.shape),))
    rows = feat.shape[0]
    n = n_series_windows(rows, seq_len, stride) if n_windows is None else int(n_windows)
    if n < 1 or (n - 1) * stride + seq_len + 3 > rows:
        raise RuntimeError("windgnn_amd.series_labels: the last of the %d windows of %d rows (stride %d) ends at row %d and "
                           "its +3 h label needs row %d, but feat has %d rows: ask for fewer windows (n_windows) or pass a "
                           "longer feat" % (n, seq_len, stride, (n - 1) * stride + seq_len - 1,
                                            (n - 1) * stride + seq_len + 2, rows))
    y = feat[:, :, LABEL_FEATURE]
    Ls = torch.cat([y[1:rows - 2], y[2:rows - 1], y[3:rows]], dim=1)          # [rows - 3, 3S]
    return Ls, Ls.unfold(0, seq_len, stride)[:n].permute(0, 2, 1)
