"""The cases of series validation (include/windgnn_series_val.h), shared by tests/test_series_val_host.py (which qualifies them on
the fp64 oracle alone) and tests/test_gpu_series_val.py.  No GPU is needed to import or to call anything here.

A case is a case of tests/series_lossfn_cases.py -- (base, how, mask, kind, delta, t_from), its shapes, draws, tables, masks and
loss formers -- and the reference is that module's: the fp64 oracle's forward on the materialised windows, the loss formed over
M = {t >= t_from, and (not masked or the label is not NaN)}.  masked follows the mask: "e" (no NaN) runs with masked = 0, "b" and
"a" with masked = 1.

    GRID       {MSE, L1, Huber 0.25} x t_from {0, 2, T - 1} x masks {e, b} on the irregular table (S 7, H 21, rows 40, T 5, n 19)
               and on the same series strided (stride 2, n 18)
    REAL       the real widths (S 34, H 102, rows 66, T 24), the three kinds from step 12 under mask a, Huber also unmasked, and
               MSE over every step
    INSTANCES  the launch arguments that are new (last_only with a spec): all nine K once each at K*_small (rows 36, T 3, n 17,
               H = 4 K), row mappings, kinds and masks alternating, from step 1
"""
import series_at_cases as sc
import series_lossfn_cases as lc

DELTA = lc.DELTA
CASES = {}


def _add(base, how, mask, kind, t_from):
    cid = "%s-%s-%s-%s-from%d" % (base, how, mask, kind, t_from)
    CASES[cid] = (base, how, mask, kind, DELTA if kind == "huber" else 0.0, t_from)
    return cid


GRID = [_add("irregular", how, mask, kind, t_from)
        for how in ("table", "stride2") for kind in ("mse", "l1", "huber") for t_from in (0, 2, 4) for mask in "eb"]
REAL = ([_add("real_widths", "table", "a", kind, 12) for kind in ("mse", "l1", "huber")] +
        [_add("real_widths", "table", "e", "huber", 12), _add("real_widths", "table", "a", "mse", 0)])
INSTANCES = [_add("K%d_small" % K, "table" if i % 2 == 0 else "stride2", "b" if i % 2 == 0 else "e", ("l1", "huber", "mse")[i % 3], 1)
             for i, K in enumerate(sc.FWD_KS)]


def reference(cid):
    return lc.reference(*CASES[cid])


def oracle_loss(q, t_from=None, divide_by=None):
    """The fp64 loss of the reference q's spec, or one of the two planted mistakes: t_from = T - 1 (a loss taken at the last step
    only), divide_by = n T H (the mean over every entry although the warm-up steps are not counted)."""
    t = q.t_from if t_from is None else t_from
    loss, _, m = lc.loss_and_dy(q.Yo, q.L.double(), q.kind, q.delta, t, q.masked)
    if divide_by is not None:
        loss = loss * m / divide_by
    return float(loss), m


def last_rows(q, wind_min, wind_max):
    """[n, H] fp64: the oracle's de-normalised last rows, Y[:, T - 1] (wind_max - wind_min) + wind_min."""
    return q.Yo[:, -1] * (wind_max - wind_min) + wind_min
