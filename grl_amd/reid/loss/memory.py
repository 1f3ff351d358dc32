"""The one place the memory criteria touch the device: OIMLoss and the cluster, proxy and hybrid memories, hard
and soft, are each a cross-entropy entry point of their own between the same three steps.

forward : ``scaled_logits``: logits = scalar * x . mem^T -- the K-blocked fp32 MFMA GEMM with the scale in its epilogue.  With a
          teacher its rows are stacked under the student's, so that ONE GEMM gives both logits.  Then the criterion's own entry
          point: loss, dlogits and the top-1 count in one launch.
backward: ``backward``: ``input_grad`` = g * scalar * dlogits . mem (`grl_oim_grad`) with the memory AS IT IS WHEN THE BACKWARD
          RUNS (oim.py:23 reads self.lut at backward time), then -- inside the backward, as upstream -- ``update``: the memory
          rows of the batch's labels blended with the batch's rows and re-normalised, by one of the three rules of ``MODES``.

No torch op computes here (the stacking is a copy) and nothing syncs with the host; there is no CPU path.

Multi-process data parallel: every rank applies the updates of ALL ranks in rank order (all_gather of the small (features,
labels) block), so the memories stay identical without a parameter broadcast."""
import ctypes as C

import torch

from grl_amd import _lib
from grl_amd._lib import ptr, MATH_F32

MODES = ('hard', 'mean', 'instance')
OG_MAX_COLS = 5120              # grl_oim_grad's limit: its 8 gradient rows live in LDS (160 KB)


def _call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, _lib.stream()), name)


def _labels(t, dev):
    if not torch.is_tensor(t):
        raise _lib.GrlHipError('labels must be a tensor')
    return t.to(device=dev, dtype=torch.int64).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# forward
def scaled_logits(x, mem, scalar, teacher=None):
    """(all logits, the student's logits) = scalar * rows . mem^T, rows = x [n, D], or x over ``teacher`` [2n, D]: one GEMM
    serves the student and the teacher, whose logits are rows n .. 2n of the first result.  Without a teacher the two are one
    tensor."""
    from grl_amd import engine
    rows = x if teacher is None else torch.cat((x, teacher))
    m, N = rows.size(0), mem.size(0)
    scale = torch.full((N,), float(scalar), dtype=torch.float32, device=x.device)
    logits = torch.empty((m, N), dtype=torch.float32, device=x.device)
    # (K-blocked: split over K, include/grl_hip.h.  The GEMM takes K % 32 == 0: another D gets zero columns -- copies, +0 to
    #  every dot product -- as the engine pads the evaluator's features; D % 32 == 0 hands over the rows and mem themselves)
    rk, mk = engine._pad_features(rows), engine._pad_features(mem)
    engine.gemm(rk, mk, logits, m, N, rk.size(1), scale=scale, math=MATH_F32, kblock=True)
    return logits, (logits if teacher is None else logits[:x.size(0)])


def ce_outputs(logits, ws_floats):
    """(loss, correct, dlogits, ws): what every cross-entropy entry point writes.  correct[0] = rows whose arg-max is the
    label (first index on ties, as the reference's topk read-out, eva_functions.py:118-131): the trainer's precision comes
    out of the same launch instead of topk / eq / sum."""
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    correct = torch.empty((), dtype=torch.float32, device=logits.device)
    return loss, correct, torch.empty_like(logits), torch.empty(ws_floats, dtype=torch.float32, device=logits.device)


def save(ctx, x, labels, dlogits, mem, momentum, scalar, mode):
    """What ``backward`` reads; ``labels`` are the memory rows the update blends the rows of ``x`` into."""
    ctx.save_for_backward(x, labels, dlogits)
    ctx.mem, ctx.momentum, ctx.scalar, ctx.mode = mem, momentum, float(scalar), mode


def top1(out):
    """(loss, logits) of a Function's (loss, logits, correct); the logits carry ``grl_top1 = (correct rows, rows)`` (device
    scalar) for ``SEQTrainer._top1``."""
    loss, logits, correct = out
    logits.grl_top1 = (correct, logits.size(0))
    return loss, logits


# ----------------------------------------------------------------------------------------------------------------------
# backward
def input_grad(dlogits, mem, gloss, scalar, x):
    """gloss * scalar * dlogits . mem, [n, D] as ``x``.  N <= 5120: one `grl_oim_grad` call.  A larger memory (MARS: 8298
    tracklets) goes through it in column blocks of 5120 -- dlogits and the memory offset by the block, ldd = N -- added up by
    `grl_axpby` in block order."""
    n, D = x.shape
    N = mem.size(0)
    g = gloss.contiguous().float()
    grad = torch.empty_like(x)
    part = torch.empty_like(x) if N > OG_MAX_COLS else None
    for j0 in range(0, N, OG_MAX_COLS):
        _call('grl_oim_grad', dlogits.data_ptr() + 4 * j0, N, mem.data_ptr() + 4 * j0 * D, ptr(g), C.c_float(scalar),
              ptr(part if j0 else grad), n, min(OG_MAX_COLS, N - j0), D)
        if j0:
            _call('grl_axpby', ptr(grad), ptr(part), ptr(grad), C.c_float(1.0), C.c_float(1.0), n * D)
    return grad


def update(mem, x, labels, momentum, mode):
    """The memory update over the (x, labels) blocks of all ranks in rank order, so that every rank applies the same global
    update.  A label outside [0, N) updates nothing.
      'instance'  every sample, in batch order: c[y] = m c[y] + (1 - m) x, renormalised (`grl_oim_update`; OIM's and CAP's rule)
      'hard'      per row present in the batch, one blend with its LEAST similar sample (`grl_cmem_update`, mode 0)
      'mean'      per row present in the batch, one blend with the mean of its samples (`grl_cmem_update`, mode 1)"""
    from grl_amd import dist as grl_dist
    xs, ys = grl_dist.gather_rank_order(x, labels)
    if mode == 'instance':
        _call('grl_oim_update', ptr(mem), ptr(xs), ptr(ys), xs.size(0), x.size(1), mem.size(0), C.c_float(momentum))
    else:
        _call('grl_cmem_update', ptr(mem), ptr(xs), ptr(ys), xs.size(0), x.size(1), mem.size(0), C.c_float(momentum),
              MODES.index(mode), None)


def backward(ctx, gloss):
    """The gradient of the inputs (None where they need none) on what ``save`` kept, then the memory update."""
    x, labels, dlogits = ctx.saved_tensors
    grad = input_grad(dlogits, ctx.mem, gloss, ctx.scalar, x) if ctx.needs_input_grad[0] else None
    update(ctx.mem, x, labels, ctx.momentum, ctx.mode)
    return grad


# ----------------------------------------------------------------------------------------------------------------------
# checks: each a ValueError that names the criterion, none a device call
def check_memory(who, name, rows, mem, num_features):
    """``mem`` is a float32 tensor [rows >= 1, num_features]; ``rows`` is the letter the message gives the row count."""
    if not (torch.is_tensor(mem) and mem.dtype == torch.float32):
        raise ValueError('%s: %s must be a float32 tensor (got %s)' % (
            who, name, mem.dtype if torch.is_tensor(mem) else type(mem).__name__))
    if mem.dim() != 2 or mem.size(0) < 1 or mem.size(1) != num_features:
        raise ValueError('%s: %s must be [%s >= 1, num_features = %d] (got %s)' % (who, name, rows, num_features, tuple(mem.shape)))


def check_table(who, name, t):
    if not (torch.is_tensor(t) and t.dtype == torch.int32):
        raise ValueError('%s: %s must be an int32 tensor (got %s)' % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))


def check_devices(who, name, mem, tables=()):
    """``mem`` is on a HIP device and every (name, tensor) of ``tables`` on the same one."""
    if not mem.is_cuda:
        raise ValueError('%s: %s must be on a HIP device (got %s)' % (who, name, mem.device))
    for tname, t in tables:
        if t.device != mem.device:
            raise ValueError('%s: %s must be on the device of the %s, %s (got %s)' % (who, tname, name, mem.device, t.device))


def check_teacher(teacher, inputs, who='SoftClusterMemoryLoss'):
    """ValueError unless ``teacher`` is a float32 tensor of ``inputs``' shape on ``inputs``' device that carries no gradient."""
    if not torch.is_tensor(teacher):
        raise ValueError('%s: teacher must be a tensor (got %s)' % (who, type(teacher).__name__))
    if tuple(teacher.shape) != tuple(inputs.shape) or teacher.dim() != 2:
        raise ValueError('%s: teacher must be [n, D] = %s, the shape of the inputs (got %s)' % (
            who, tuple(inputs.shape), tuple(teacher.shape)))
    if teacher.dtype != torch.float32:
        raise ValueError('%s: teacher must be float32 (got %s)' % (who, teacher.dtype))
    if teacher.device != inputs.device:
        raise ValueError('%s: teacher must be on the device of the inputs, %s (got %s)' % (who, inputs.device, teacher.device))
    if teacher.requires_grad:
        raise ValueError('%s: teacher must carry no gradient (compute it under torch.no_grad() or detach it)' % who)


def soft_target(who, inputs, teacher, soft_weight):
    """(teacher rows, w) for a soft entry point, or (None, 0.0) where the hard one serves: no teacher, or ``soft_weight`` 0 --
    the base criterion's launches, the same bits."""
    w = float(soft_weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError('%s: soft_weight must be in [0, 1] (got %r)' % (who, soft_weight))
    if teacher is None or w == 0.0:
        return None, 0.0
    check_teacher(teacher, inputs, who)
    return teacher.contiguous(), w
