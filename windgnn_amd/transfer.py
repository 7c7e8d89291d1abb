"""Moving a trained model to another station network.

conv1 / conv2 of the reference's model are 13 x 13 (+ 13): they act on one station's features and do not depend on the number
of stations S.  The GRU tensors do ([3H, S * 13], [3H, H], H = 3S): they must be trained again on the new network.
adopt_convs copies the convolutions of a trained model into a model of any S; TrainStep(trainable="gru") then trains the GRU
under the frozen convolutions without paying for their backward, and set_trainable("all") may follow for a few steps on
everything ("Moving a trained model to another station network")."""
from __future__ import annotations

import os

import torch

from .functional import PARAM_ORDER
from .modules import GCN_GRU, NUM_FEATURES

CONV_KEYS = PARAM_ORDER[:4]         # conv1.weight, conv1.bias, conv2.weight, conv2.bias
_SHAPES = {"conv1.weight": (NUM_FEATURES, NUM_FEATURES), "conv1.bias": (NUM_FEATURES,),
           "conv2.weight": (NUM_FEATURES, NUM_FEATURES), "conv2.bias": (NUM_FEATURES,)}


def _widths(who, model):
    if not isinstance(model, GCN_GRU):
        raise TypeError("windgnn_amd: adopt_convs: %s is %s, not a windgnn_amd.GCN_GRU" % (who, type(model).__name__))
    if not model.fused:
        raise RuntimeError("windgnn_amd: adopt_convs: %s has convolutions of %s -> %s, not the reference model's 13 -> 13 -> 13 "
                           "(src/main.py:41); only those carry over between station networks here"
                           % (who, " -> ".join(str(n) for n in model.conv1.weight.shape), model.conv2.weight.shape[1]))


def adopt_convs(model, source):
    """Copy conv1.weight, conv1.bias, conv2.weight and conv2.bias of `source` into `model`, whatever the source's number of
    stations S and GRU width H; the GRU tensors of `model` are not touched.  source: a GCN_GRU, a state_dict (the reference's
    keys; further keys, the GRU's among them, are ignored) or a path torch.load reads one from.  Raises if either model's
    widths are not 13 / 13, or if the dict lacks one of the four tensors or holds one of another shape -- before anything is
    written.  Returns the list of copied keys.

    The copy goes through the nn.Parameters in place, under torch.no_grad(): torch's version counters tell a TrainStep made
    earlier on `model` that its parameters were written, and it rebuilds its staged W_ih images on the next step by itself --
    no tr.refresh() is needed (that call is for writes torch does not count, such as p.data.copy_)."""
    _widths("model", model)
    if isinstance(source, (str, os.PathLike)):
        source = torch.load(source, map_location="cpu")
    if isinstance(source, torch.nn.Module):
        _widths("source", source)
        source = source.state_dict()
    if not hasattr(source, "keys"):
        raise TypeError("windgnn_amd: adopt_convs: source must be a GCN_GRU, a state_dict or a path to one, got %s"
                        % type(source).__name__)
    missing = [k for k in CONV_KEYS if k not in source]
    if missing:
        raise KeyError("windgnn_amd: adopt_convs: the source lacks %s" % ", ".join(missing))
    for k in CONV_KEYS:
        if tuple(source[k].shape) != _SHAPES[k]:
            raise RuntimeError("windgnn_amd: adopt_convs: the source's %s is %s, not %s: only the reference model's widths "
                               "13 / 13 carry over" % (k, tuple(source[k].shape), _SHAPES[k]))
    mine = dict(model.named_parameters())
    with torch.no_grad():
        for k in CONV_KEYS:
            mine[k].copy_(torch.as_tensor(source[k]))
    return list(CONV_KEYS)
