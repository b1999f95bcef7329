"""Shared by the batch-statistics BatchNorm tests: the train-mode evaluation of the CPU oracle.

A frozen backbone left in .train() (ContextPose_mpi/run_3dhp.py:31-35 never calls backbone.eval()) normalises every BatchNorm2d with the
statistics of the batch and moves running_mean / running_var with momentum 0.1.  capf_oracle evaluates every BatchNorm through the module
attribute capf_oracle._bn; batch_stat_bn() swaps that attribute for F.batch_norm(..., training=True) while it is open, which reproduces the
reference backbone under .train() bit for bit (tests/golden/mpi_bn_train_w32_64x64.npz pins that, tools/make_bn_train_golden.py writes it).
The running statistics of the state dict the oracle is given are updated IN PLACE, in the dict's own dtype (fp32 or fp64);
num_batches_tracked is the caller's to count, as it is for the library."""
import contextlib

import torch
import torch.nn.functional as F

import capf_oracle as oracle

MOMENTUM = 0.1        # nn.BatchNorm2d's default; pose_hrnet.py BN_MOMENTUM


@contextlib.contextmanager
def batch_stat_bn(momentum=MOMENTUM):
    """While open, every BatchNorm of capf_oracle normalises with batch statistics and updates P[...running_mean / running_var] in place;
    restored on exit, whatever happens inside."""
    saved = oracle._bn

    def bn_train(P, name, x):
        return F.batch_norm(x, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                            True, momentum, oracle.BN_EPS)

    oracle._bn = bn_train
    try:
        yield
    finally:
        oracle._bn = saved


def backbone_keys(sd):
    """names of the backbone's BatchNorm layers ('backbone....bn1', ...) in state-dict order"""
    return [k[:-len(".running_mean")] for k in sd if k.startswith("backbone.") and k.endswith(".running_mean")]


def to_double(sd):
    """an fp64 copy of a state dict (integer buffers kept)"""
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def clone_sd(sd):
    return {k: v.clone() for k, v in sd.items()}


def train_maps(sd, images_nhwc, backbone="hrnet_32", momentum=MOMENTUM):
    """The four context maps (NCHW, the dict's dtype) of one train-mode backbone forward; sd's running statistics move."""
    # (contiguous NCHW, as the reference feeds its backbone: a permuted view would send ATen down its channels-last kernels, another summation order)
    x = images_nhwc.permute(0, 3, 1, 2).contiguous().to(next(v for k, v in sd.items() if k.endswith("conv1.weight")).dtype)
    with batch_stat_bn(momentum), torch.no_grad():
        return oracle.hrnet_forward(sd, x)


def rel_dist(a, b):
    """max |a - b| over max |b|"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()
