"""ctypes binding of libwindgnn_hip.so (the C ABI declared in include/windgnn.h, windgnn_optim.h, windgnn_sched.h,
windgnn_eval.h, windgnn_best.h, windgnn_series.h, windgnn_series_train.h, windgnn_series_at.h, windgnn_series_masked.h,
windgnn_series_lossfn.h and windgnn_series_val.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  If the shared object is
missing or a call fails this module raises, loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# WGNN_LIB: another build of the SAME library (same-box A/B timing of kernel variants, tools/exp); never a different backend
LIB_PATH = os.environ.get("WGNN_LIB") or os.path.join(_HERE, "csrc", "libwindgnn_hip.so")

MATH_F32 = 0
MATH_F16X3 = 1
MATH_F16 = 2
MATH_F16X3G = 3       # f16x3 whose backward gate gradients travel as one fp16 plane from B*T >= 4096 (include/windgnn.h)
ADJ_DENSE = 0
ADJ_CSR = 1
IO_F32, IO_F16, IO_BF16 = 0, 1, 2   # wgnn_io: element type of X, Y and the labels
STEP_MAX_B = 256            # wgnn_fwd_state: T == 1 calls up to this batch (dense A, fp32 I/O, H <= 128) run ONE kernel
STATUS_BYTES = 256          # WGNN_STATUS_BYTES: status block at the start of every workspace
OPT_FUSED_FWD = 0           # WGNN_OPT_FUSED_FWD (wgnn_set_option): 0 never / 1 stash-less forwards / 2 every supported forward
OPT_BIG_GEMM = 4            # WGNN_OPT_BIG_GEMM: 1 (default) the 256 x 256-tile kernel for large NT plane products / 0 off (keys 1, 2, 3, 5 are retired)
OPT_TN_MERGED = 6           # WGNN_OPT_TN_MERGED: 1 (default) one launch for both GRU weight-gradient GEMMs (dW_hh reads h from fp32 Y, no Y planes) / 0 one each; same bits; not to be changed between a forward and its backward


class Dims(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("S", C.c_int32), ("F", C.c_int32), ("H", C.c_int32),
                ("math", C.c_int32), ("adj_format", C.c_int32), ("nnz", C.c_int32), ("io", C.c_int32)]


_SLOTS = ("conv1_weight", "conv1_bias", "conv2_weight", "conv2_bias", "w_ih", "w_hh", "b_ih", "b_hh")


class Params(C.Structure):
    # wgnn_params: the 8 tensors + the optional caller-kept images of W_ih (NULL = rebuilt inside every call)
    _fields_ = [(n, C.c_void_p) for n in _SLOTS] + [("prepared", C.c_void_p)]


class Grads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _SLOTS]


class Adam(C.Structure):
    # wgnn_adam
    _fields_ = [("exp_avg", Grads), ("exp_avg_sq", Grads), ("step", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float)]


BWD_DEFER = 16              # WGNN_BWD_DEFER
FINISH_ADAM_GRU = 16        # WGNN_FINISH_ADAM_GRU / _CONV: wgnn_finish's optimiser step of one tensor family only
FINISH_ADAM_CONV = 32
ROWS_IH, ROWS_HH, ROWS_STATE = 1, 2, 4   # WGNN_ROWS_*: wgnn_bwd_rows / wgnn_finish_rows (row ranges of one GRU pair)


EXPORTS = {
    "wgnn_version": (C.c_int, []),
    "wgnn_strerror": (C.c_char_p, [C.c_int]),
    "wgnn_set_option": (C.c_int, [C.c_int, C.c_int]),
    "wgnn_get_option": (C.c_int, [C.c_int]),
    "wgnn_workspace_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "wgnn_stash_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "wgnn_fwd": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_fwd_loss": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_fwd_last": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_float, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_fwd_state": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_state_stash_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "wgnn_fwd_state_stash": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_bwd_state_part": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_int]),
    "wgnn_bwd": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                           C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_bwd_part": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "wgnn_bwd_mse_part": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_int]),
    "wgnn_finish": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(Grads), C.c_int, C.POINTER(Adam), C.c_void_p,
                              C.c_size_t, C.c_void_p]),
    "wgnn_bwd_rows_align": (C.c_int, [C.POINTER(Dims)]),
    "wgnn_bwd_rows": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.c_void_p, C.POINTER(Grads), C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_finish_rows": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(Grads), C.c_int, C.c_int, C.c_int,
                                   C.POINTER(Adam), C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_prepared_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "wgnn_prepare_weights": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_gcn_layer_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "wgnn_gcn_layer_fwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "wgnn_gcn_layer_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "wgnn_gru_fwd": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]),
    "wgnn_gru_bwd": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(Grads), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_gcn_layer_csr_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "wgnn_gcn_layer_csr_fwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "wgnn_gcn_layer_csr_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "wgnn_mse_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_make_windows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wgnn_predict_last": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                    C.c_void_p]),
    "wgnn_profile_enable": (C.c_int, [C.c_int]),
    "wgnn_profile_read": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wgnn_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
}

# include/windgnn_optim.h: clipping by the global gradient norm inside the step tail (a second header and a second table:
# include/windgnn.h and EXPORTS stay as they are)
OPTIM_VERSION = 1           # WGNN_OPTIM_VERSION
CLIP_TOTAL, CLIP_COEF = 0, 1   # float slots of the `clip` buffer: the gradient's L2 norm, min(1, max_norm / (norm + 1e-6))
EXPORTS_OPTIM = {
    "wgnn_optim_version": (C.c_int, []),
    "wgnn_clip_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "wgnn_finish_norm": (C.c_int, [C.POINTER(Dims), C.POINTER(Grads), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "wgnn_finish_clipped": (C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.POINTER(Grads), C.POINTER(Adam), C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/windgnn_sched.h: host-only schedule queries (a third header and table, as above)
class TnSplitInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sk_ih", "sk_hh", "kchunk_ih", "kchunk_hh", "merged", "workgroups")]


EXPORTS_SCHED = {
    "wgnn_tn_split": (C.c_int, [C.POINTER(Dims), C.c_int, C.POINTER(TnSplitInfo)]),
}

# include/windgnn_eval.h: the test loop's statistics accumulated on the device (a fourth header and table, as above)
EVAL_VERSION = 1            # WGNN_EVAL_VERSION
EVAL_ROWS = ("n", "sum_e2", "sum_abs_e", "sum_a", "sum_a2")   # the fp64 rows [H] at the start of `acc`, in this order
EXPORTS_EVAL = {
    "wgnn_eval_version": (C.c_int, []),
    "wgnn_eval_bytes": (C.c_size_t, [C.c_int32]),
    "wgnn_eval_accum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "wgnn_eval_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
}

# include/windgnn_best.h: the reference's keep-the-best-model rule on the device (a fifth header and table, as above)
BEST_VERSION = 1            # WGNN_BEST_VERSION
# the public words of the record: name -> (byte offset, torch dtype name)
BEST_WORDS = {"best_loss": (0, "float64"), "best_step": (8, "int64"), "calls": (16, "int64"), "improvements": (24, "int64"),
              "improved": (32, "int32")}
EXPORTS_BEST = {
    "wgnn_best_version": (C.c_int, []),
    "wgnn_best_bytes": (C.c_size_t, []),
    "wgnn_best_init": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "wgnn_keep_best": (C.c_int, [C.POINTER(Dims), C.c_void_p, C.POINTER(Params), C.POINTER(Params), C.c_int64, C.c_void_p,
                                 C.c_void_p]),
}

# include/windgnn_series.h: the model on the sliding windows of one series (a sixth header and table, as above)
SERIES_VERSION = 1          # WGNN_SERIES_VERSION


class SeriesDims(C.Structure):
    # wgnn_series_dims
    _fields_ = [(n, C.c_int32) for n in ("rows", "T", "stride", "n", "S", "F", "H", "math", "adj_format", "nnz", "io")]


EXPORTS_SERIES = {
    "wgnn_series_version": (C.c_int, []),
    "wgnn_series_workspace_bytes": (C.c_size_t, [C.POINTER(SeriesDims)]),
    "wgnn_series_stash_bytes": (C.c_size_t, [C.POINTER(SeriesDims)]),
    "wgnn_series_fwd": (C.c_int, [C.POINTER(SeriesDims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_fwd_last": (C.c_int, [C.POINTER(SeriesDims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_float, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_bwd": (C.c_int, [C.POINTER(SeriesDims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/windgnn_series_train.h: the MSE loss fused into the series recurrences (a seventh header and table, as above)
SERIES_TRAIN_VERSION = 1    # WGNN_SERIES_TRAIN_VERSION
EXPORTS_SERIES_TRAIN = {
    "wgnn_series_train_version": (C.c_int, []),
    "wgnn_series_loss_bytes": (C.c_size_t, [C.POINTER(SeriesDims)]),
    "wgnn_series_status_offset": (C.c_size_t, [C.POINTER(SeriesDims)]),
    "wgnn_series_fwd_loss": (C.c_int, [C.POINTER(SeriesDims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_bwd_mse": (C.c_int, [C.POINTER(SeriesDims), C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Grads), C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
}

# include/windgnn_series_at.h: series mode on windows at a table of start rows (an eighth header and table, as above)
SERIES_AT_VERSION = 1       # WGNN_SERIES_AT_VERSION
STATUS_WINDOW_START = 16    # WGNN_STATUS_WINDOW_START
_SD = C.POINTER(SeriesDims)
EXPORTS_SERIES_AT = {
    "wgnn_series_at_version": (C.c_int, []),
    "wgnn_series_at_workspace_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_at_stash_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_at_loss_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_at_status_offset": (C.c_size_t, [_SD]),
    "wgnn_series_fwd_at": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_fwd_last_at": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_float, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_bwd_at": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(Grads), C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_fwd_loss_at": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_bwd_mse_at": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Grads),
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/windgnn_series_masked.h: series training / evaluation through missing labels, NaN = no label (a ninth header and table)
SERIES_MASKED_VERSION = 1   # WGNN_SERIES_MASKED_VERSION
STATUS_NO_LABELS = 32       # WGNN_STATUS_NO_LABELS
EXPORTS_SERIES_MASKED = {
    "wgnn_series_masked_version": (C.c_int, []),
    "wgnn_series_masked_loss_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_fwd_loss_masked": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_series_bwd_mse_masked": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Grads),
                                             C.c_void_p, C.c_size_t, C.c_void_p]),
    "wgnn_eval_accum_series": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/windgnn_series_lossfn.h: series training on a loss spec -- MSE / L1 / Huber, from a warm-up step on (a tenth header and table)
SERIES_LOSSFN_VERSION = 1   # WGNN_SERIES_LOSSFN_VERSION
LOSS_MSE, LOSS_L1, LOSS_HUBER = 0, 1, 2
LOSS_KINDS = {"mse": LOSS_MSE, "l1": LOSS_L1, "huber": LOSS_HUBER}


class LossFn(C.Structure):
    """wgnn_lossfn"""
    _fields_ = [("kind", C.c_int32), ("delta", C.c_float), ("t_from", C.c_int32), ("masked", C.c_int32)]


EXPORTS_SERIES_LOSSFN = {
    "wgnn_series_lossfn_version": (C.c_int, []),
    "wgnn_series_lossfn_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_fwd_lossfn": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64,
                                         C.POINTER(LossFn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "wgnn_series_bwd_lossfn": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_float, C.POINTER(LossFn), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(Grads), C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/windgnn_series_val.h: the held-out loss of a spec, forward-only, accumulated on the device (an eleventh header and table)
SERIES_VAL_VERSION = 1      # WGNN_SERIES_VAL_VERSION
STATUS_NO_LOSS_STATS = 8    # WGNN_STATUS_NO_LOSS_STATS
# the public words of the record: name -> (byte offset, torch dtype name); `count` is a uint64 read as int64
VAL_WORDS = {"sum": (0, "float64"), "count": (8, "int64"), "mean": (16, "float64"), "max_abs": (24, "float32"),
             "loss": (28, "float32"), "calls": (32, "int64"), "passes": (40, "int64"), "stale": (48, "int64")}
EXPORTS_SERIES_VAL = {
    "wgnn_series_val_version": (C.c_int, []),
    "wgnn_val_bytes": (C.c_size_t, []),
    "wgnn_val_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wgnn_val_begin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wgnn_series_val_workspace_bytes": (C.c_size_t, [_SD]),
    "wgnn_series_val": (C.c_int, [_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64,
                                  C.POINTER(LossFn), C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "wgnn_val_close": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library or raise.  Never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "windgnn_amd: %s is missing. Build it with `python -m windgnn_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError here = ABI mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.wgnn_version() < 122:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old")
    if not hasattr(lib, "wgnn_optim_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_optim.h (no wgnn_optim_version): rebuild it with "
                           "`python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_OPTIM.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in EXPORTS_SCHED.items():
        if not hasattr(lib, name):
            raise RuntimeError("windgnn_amd: %s predates include/windgnn_sched.h (no %s): rebuild it with "
                               "`python -m windgnn_amd.build --force`" % (LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_eval_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_eval.h (no wgnn_eval_version): rebuild it with "
                           "`python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_EVAL.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_best_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_best.h (no wgnn_best_version): rebuild it with "
                           "`python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_BEST.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_series_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series.h (no wgnn_series_version): rebuild it with "
                           "`python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_series_train_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series_train.h (no wgnn_series_train_version): rebuild it "
                           "with `python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES_TRAIN.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_series_at_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series_at.h (no wgnn_series_at_version): rebuild it "
                           "with `python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES_AT.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not hasattr(lib, "wgnn_series_masked_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series_masked.h (no wgnn_series_masked_version): rebuild it "
                           "with `python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES_MASKED.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.wgnn_series_masked_version() < SERIES_MASKED_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_masked_version %d < %d)"
                           % (lib.wgnn_series_masked_version(), SERIES_MASKED_VERSION))
    if not hasattr(lib, "wgnn_series_lossfn_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series_lossfn.h (no wgnn_series_lossfn_version): rebuild it "
                           "with `python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES_LOSSFN.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.wgnn_series_lossfn_version() < SERIES_LOSSFN_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_lossfn_version %d < %d)"
                           % (lib.wgnn_series_lossfn_version(), SERIES_LOSSFN_VERSION))
    if not hasattr(lib, "wgnn_series_val_version"):
        raise RuntimeError("windgnn_amd: %s predates include/windgnn_series_val.h (no wgnn_series_val_version): rebuild it "
                           "with `python -m windgnn_amd.build --force`" % LIB_PATH)
    for name, (res, args) in EXPORTS_SERIES_VAL.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.wgnn_series_val_version() < SERIES_VAL_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_val_version %d < %d)"
                           % (lib.wgnn_series_val_version(), SERIES_VAL_VERSION))
    if lib.wgnn_series_at_version() < SERIES_AT_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_at_version %d < %d)"
                           % (lib.wgnn_series_at_version(), SERIES_AT_VERSION))
    if lib.wgnn_series_train_version() < SERIES_TRAIN_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_train_version %d < %d)"
                           % (lib.wgnn_series_train_version(), SERIES_TRAIN_VERSION))
    if lib.wgnn_series_version() < SERIES_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_series_version %d < %d)"
                           % (lib.wgnn_series_version(), SERIES_VERSION))
    if lib.wgnn_best_version() < BEST_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_best_version %d < %d)"
                           % (lib.wgnn_best_version(), BEST_VERSION))
    if lib.wgnn_eval_version() < EVAL_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_eval_version %d < %d)"
                           % (lib.wgnn_eval_version(), EVAL_VERSION))
    if lib.wgnn_optim_version() < OPTIM_VERSION:
        raise RuntimeError("windgnn_amd: libwindgnn_hip.so is too old (wgnn_optim_version %d < %d)"
                           % (lib.wgnn_optim_version(), OPTIM_VERSION))
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().wgnn_strerror(status).decode()
        raise RuntimeError("windgnn_amd: %s failed: %s (status %d)" % (what, msg, status))


def set_option(key: int, value: int) -> int:
    """wgnn_set_option: returns the previous value; raises on an unknown key / value."""
    prev = load().wgnn_set_option(key, value)
    if prev < 0:
        check(prev, "wgnn_set_option(%d, %d)" % (key, value))
    return prev


def get_option(key: int) -> int:
    v = load().wgnn_get_option(key)
    if v < 0:
        check(v, "wgnn_get_option(%d)" % key)
    return v


def tn_split(dims: Dims, state: bool = False) -> TnSplitInfo:
    """wgnn_tn_split: the split-K factors of the two GRU weight-gradient GEMMs for `dims`."""
    info = TnSplitInfo()
    check(load().wgnn_tn_split(C.byref(dims), 1 if state else 0, C.byref(info)), "wgnn_tn_split")
    return info


def profile_enable(on: bool) -> None:
    check(load().wgnn_profile_enable(1 if on else 0), "wgnn_profile_enable")


def profile_read():
    """[{name, ms, launches, flops, bytes}] accumulated since profile_enable(True)."""
    lib = load()
    out = []
    i = 0
    while True:
        name = C.create_string_buffer(128)
        ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        if lib.wgnn_profile_read(i, name, 128, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) != 0:
            break
        out.append({"name": name.value.decode(), "ms": ms.value, "launches": n.value, "flops": fl.value,
                    "bytes": by.value})
        i += 1
    return out
