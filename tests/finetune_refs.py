"""References for fine-tuning with frozen BatchNorm statistics and frozen parameters, shared by tests/test_finetune_cpu.py (are the
formulas autograd's, can the bounds see a dropped row, do the optimiser's ranges cover exactly the trainable slots?) and the GPU tests
(tests/test_gpu_finetune_kernels.py, tests/test_gpu_finetune.py).  Nothing here touches a GPU.

The backward of a BatchNorm that normalises with its running statistics (nn.BatchNorm2d in eval mode):
    g = dy [relu_out > 0],  dz = g gamma invstd,  dbeta = sum g,  dgamma = sum g (z - mean) invstd
with mean = running_mean and invstd = 1 / sqrt(running_var + eps) as float32 values handed to the kernel.  Bounds, derived and not
fitted: dz has two float32 roundings (gamma * invstd, then * g): 3 u |dz| covers them to first order with room for the second-order
term; the sums carry the summation bound of tests/step_kernel_refs.py::bn_bwd_sums_ref -- the kernel walks the rows with the same
workgroup mapping as fp_bn_bwd's reduction (launch_regimes.bn_chain), k = 0 roundings inside a term of dbeta, k = 3 for dgamma.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from tests import launch_regimes as LR
from tests import step_kernel_refs as SR
from tests.step_kernel_refs import bn_inputs, last_row_mask, ratio      # noqa: F401  (re-exported: the GPU tests take them from here)

U = LR.U
EPS = SR.EPS


def frozen_stats(inp):
    """the float32 (mean, invstd) a frozen-statistics forward leaves for the backward: running_mean, 1 / sqrt(running_var + eps)"""
    return inp["rm"].clone(), (1.0 / torch.sqrt(inp["rv"] + EPS)).float()


def frozen_bn_bwd_ref(inp, relu_out, keep=None, mean=None, invstd=None, ro=None):
    """-> (ref, bound) dicts over dz [M][C], dbeta, dgamma [C] and g [M][C] (exact: bound 0), in float64 from the float32 inputs.
    mean / invstd: the statistics (default: frozen_stats(inp)); ro: the ReLU output whose sign masks dy (default inp["ro"]);
    keep: a row mask -- the sums over a subset of the rows (the sensitivity test drops the last row)"""
    m32, i32 = frozen_stats(inp)
    mean = m32.double() if mean is None else mean.double()
    invstd = i32.double() if invstd is None else invstd.double()
    z, dy, gamma = inp["z"].double(), inp["dy"].double(), inp["gamma"].double()
    mask = ((inp["ro"] if ro is None else ro) > 0).double()
    g = dy * mask if relu_out else dy
    dz = g * (gamma * invstd)
    t2 = g * ((z - mean) * invstd)
    gs, t2s = (g, t2) if keep is None else (g[keep], t2[keep])
    L = LR.bn_chain(*inp["z"].shape)
    s1, s2 = gs.sum(0), t2s.sum(0)
    ref = {"dz": dz, "g": g, "dbeta": s1, "dgamma": s2}
    bound = {"dz": 3 * U * dz.abs(), "g": torch.zeros_like(g), "dbeta": LR.sum_bound(L, 0, gs.abs().sum(0), s1),
             "dgamma": LR.sum_bound(L, 3, t2s.abs().sum(0), s2)}
    return ref, bound


def frozen_bn_autograd(inp):
    """torch.autograd through relu(F.batch_norm(z, running_mean, running_var, gamma, beta, training=False)) in float64 with upstream
    gradient dy -> ({dz, dgamma, dbeta}, the ReLU output, the float64 invstd autograd used)"""
    z = inp["z"].double().requires_grad_(True)
    gamma, beta = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    rm, rv = inp["rm"].double(), inp["rv"].double()
    y = F.relu(F.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, False, 0.1, EPS))
    dz, dg, db = torch.autograd.grad(y, (z, gamma, beta), inp["dy"].double())
    return {"dz": dz, "dgamma": dg, "dbeta": db}, y.detach(), (rv + EPS) ** -0.5


# ---- the whole network with frozen statistics ----------------------------------------------------------------------------------------
def oracle_grads_eval(P, B, cpu_batch, dtype, fix_batch=None, relu_decisions=None):
    """tests/parity.py::oracle_grads with the encoder's BatchNorms on their running statistics: one forward of the CPU oracle with
    training=False + loss + autograd in `dtype` -> (outputs, losses, {name: grad}, batch used); the buffers B are not written"""
    from oracle import restatement as R
    Pd = OrderedDict((k, v.to(dtype).clone().requires_grad_(not R.is_dead_param(k))) for k, v in P.items())
    Bd = OrderedDict((k, v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in B.items())
    out = R.footprint_network(cpu_batch["image"].to(dtype), Pd, Bd, False, relu_decisions=relu_decisions)
    used = cpu_batch if fix_batch is None else fix_batch(cpu_batch, out)
    losses, _ = R.loss_manager(out, OrderedDict((k, v.to(dtype)) for k, v in used.items()))
    losses["loss"].backward()
    grads = OrderedDict((k, p.grad) for k, p in Pd.items())
    return {k: v.detach() for k, v in out.items()}, losses, grads, used


def decoder_grads64(P, feats_nchw, cpu_batch, grads=True):
    """float64 decoders + loss on GIVEN encoder features (the engine's own saved ones, NCHW) -> ({name: grad} of every live decoder
    parameter, the outputs); grads=False: the outputs alone (they do not depend on the targets: what tie_free_batch needs)"""
    from oracle import restatement as R
    Pd = OrderedDict((k, v.double().clone().requires_grad_(True)) for k, v in P.items() if "decoder" in k and not R.is_dead_param(k))
    feats = [f.double() for f in feats_nchw]
    m = R.skip_decoder(feats, Pd, "mask_decoder", False)
    d = R.skip_decoder(feats, Pd, "depth_decoder", True)
    out = OrderedDict((k, torch.cat([m[k], d[k]], 1)) for k in m)
    if not grads:
        return None, {k: v.detach() for k, v in out.items()}
    losses, _ = R.loss_manager(out, OrderedDict((k, v.double()) for k, v in cpu_batch.items()))
    losses["loss"].backward()
    return OrderedDict((k, p.grad) for k, p in Pd.items()), {k: v.detach() for k, v in out.items()}


# ---- the optimiser's ranges ----------------------------------------------------------------------------------------------------------
def flat_layout(shapes):
    """offsets of tensors of `shapes` in the engine's flat buffers (every slot padded to 16 bytes) -> (offsets, total)"""
    offs, total = [], 0
    for s in shapes:
        n = 1
        for d in s:
            n *= d
        offs.append(total)
        total += (n + 3) // 4 * 4
    return offs, total


def trainable_ranges(offsets, total, flags):
    """the optimiser's rule (footprints_amd/engine.py::trainable_ranges), as the pure function it is"""
    from footprints_amd.engine import trainable_ranges as fn
    return fn(offsets, total, flags)


def live_shapes():
    """(names, shapes) of the 196 live tensors in flat-buffer order (module order of the reference's state_dict, dead decoder BN left out)"""
    from oracle import restatement as R
    live = [(k, tuple(sh)) for k, sh, kind in R.state_spec() if kind in ("conv_w", "conv_b", "bn_w", "bn_b") and not R.is_dead_param(k)]
    return [k for k, _ in live], [sh for _, sh in live]
