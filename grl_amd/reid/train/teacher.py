"""Mean teacher for unsupervised training on MI355X (Mean Teacher, Tarvainen & Valpola 2017; MMT, Ge et al.
2020): a second copy of the CNN and the Siamese head that holds the exponential moving average of the student's weights,
gives the soft targets of ``SoftClusterMemoryLoss`` and ``SoftTripletLoss`` and the rows ``InstanceContrastLoss`` contrasts the
batch against, and is the model one evaluates and clusters with.

``MeanTeacher.update()`` is ONE `grl_ema_update` launch over a device table of every float32 parameter and buffer of both
modules (built once per model), then ``engine.touch_state`` on both copies: the kernel writes through raw pointers, which
torch's version counters never see, and the packed eval plans (folded BatchNorms, re-laid weights) must be rebuilt before the
teacher's next forward.  ``MeanTeacherSEQTrainer`` is SEQTrainer with the teacher's rows handed to its identity criteria and
the update hooked behind ``optimizer.step()``; ``MeanTeacherHybridSEQTrainer`` and ``MeanTeacherCameraSEQTrainer`` are the same
on ``HybridSEQTrainer`` and ``CameraSEQTrainer``, all three through ``MeanTeacherMixin``.  There is no CPU path."""
import copy
import ctypes as C

import torch

from grl_amd import dist as grl_dist
from grl_amd._lib import ptr, GrlEmaEntry, EMA_CHUNK
from grl_amd.reid.loss import (SoftClusterMemoryLoss, SoftHybridMemoryLoss, SoftProxyMemoryLoss, SoftTripletLoss,
                               InstanceContrastLoss)
from grl_amd.reid.loss.ins_contrast import check_ins_weights, check_temperature
from grl_amd.reid.loss.oim import _call
from grl_amd.reid.train.camera import CameraSEQTrainer
from grl_amd.reid.train.hybrid import HybridSEQTrainer
from grl_amd.reid.train.trainer import SEQTrainer


def ema_alpha(step, alpha):
    """MMT's ramp: a = min(1 - 1 / (step + 1), alpha), ``step`` counted from 0 -- the first update is a copy."""
    return min(1.0 - 1.0 / (step + 1), alpha)


def ema_tensors(student, teacher, who='MeanTeacher'):
    """[(name, teacher tensor, student tensor)] over every floating-point parameter and buffer of the two modules (same
    class, same names), each name once.  Integer buffers (``num_batches_tracked``) are left out: they are copied when the
    teacher is made and the eval forward never reads them."""
    out, seen = [], set()
    s_all = dict(list(student.named_parameters()) + list(student.named_buffers()))
    for name, t in list(teacher.named_parameters()) + list(teacher.named_buffers()):
        if name in seen or not torch.is_floating_point(t):
            continue
        seen.add(name)
        if name not in s_all:
            raise ValueError('%s: the student has no tensor %r' % (who, name))
        out.append((name, t, s_all[name]))
    return out


def check_ema_pairs(pairs, who='MeanTeacher'):
    """ValueError unless every (name, dst, src) is a pair of contiguous float32 tensors of one shape on one HIP device whose
    storage no destination shares with any other tensor of the list.  No device call."""
    for name, d, s in pairs:
        for role, t in (('teacher', d), ('student', s)):
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise ValueError('%s: %s tensor %r must be float32 (got %s)' % (
                    who, role, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
            if not t.is_contiguous():
                raise ValueError('%s: %s tensor %r must be contiguous (strides %s for shape %s)' % (
                    who, role, name, tuple(t.stride()), tuple(t.shape)))
        if tuple(d.shape) != tuple(s.shape):
            raise ValueError('%s: tensor %r is %s in the teacher and %s in the student' % (
                who, name, tuple(d.shape), tuple(s.shape)))
    src_storage = {}
    for name, d, s in pairs:
        if s.numel():
            src_storage[s.untyped_storage().data_ptr()] = name
    spans = []
    for name, d, s in pairs:
        if not d.numel():
            continue
        key = d.untyped_storage().data_ptr()
        if key in src_storage:
            raise ValueError('%s: teacher tensor %r shares its storage with the student tensor %r: the teacher must be a '
                             'copy' % (who, name, src_storage[key]))
        spans.append((d.data_ptr(), d.data_ptr() + 4 * d.numel(), name))
    spans.sort()
    for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
        if lo < hi:                                        # every element has one writer
            raise ValueError('%s: teacher tensors %r and %r overlap in memory' % (who, a, b))
    for name, d, s in pairs:
        for role, t in (('teacher', d), ('student', s)):
            if not t.is_cuda:
                raise ValueError('%s: %s tensor %r must be on a HIP device (got %s)' % (who, role, name, t.device))
        if d.device != s.device:
            raise ValueError('%s: tensor %r is on %s in the teacher and on %s in the student' % (who, name, d.device, s.device))


def ema_table(pairs):
    """(GrlEmaEntry array, chunk_first list [count + 1]) of the pairs that hold an element, on the host."""
    live = [(d, s) for _, d, s in pairs if d.numel()]
    arr = (GrlEmaEntry * max(len(live), 1))()
    first = [0]
    for i, (d, s) in enumerate(live):
        arr[i].dst, arr[i].src, arr[i].numel = d.data_ptr(), s.data_ptr(), d.numel()
        first.append(first[-1] + (d.numel() + EMA_CHUNK - 1) // EMA_CHUNK)
    return arr, first, len(live)


class MeanTeacher(object):
    """``MeanTeacher(cnn_model, siamese_model, alpha=0.999)``: deep copies of the two modules in ``eval()`` without
    gradients, and ``update()`` = one launch that moves every float32 parameter and buffer of the copies (the BatchNorm running
    statistics included, as ``AveragedModel(use_buffers=True)``) towards the student's:
    teacher = a teacher + (1 - a) student with a = min(1 - 1 / (step + 1), alpha).
    ``siamese_model_uncorr`` has no parameter on the identity path and needs no copy."""

    def __init__(self, cnn_model, siamese_model, alpha=0.999):
        if not 0.0 <= float(alpha) < 1.0:
            raise ValueError('MeanTeacher: alpha must be in [0, 1) (got %r)' % (alpha,))
        self.alpha = float(alpha)
        self.step = 0
        self.student = (getattr(cnn_model, 'module', cnn_model), siamese_model)
        self.cnn, self.siamese = (copy.deepcopy(m) for m in self.student)
        for m in (self.cnn, self.siamese):
            m.eval()
            m.requires_grad_(False)
            for p in m.parameters():
                p.grad = None
            m.__dict__.pop('_grl_weight_prep', None)       # (a copied train-step plan points at the student's buffers)
        self._build()

    def _build(self):
        self.pairs = [p for t, s in zip((self.cnn, self.siamese), self.student) for p in ema_tensors(s, t)]
        check_ema_pairs(self.pairs)
        arr, first, self.count = ema_table(self.pairs)
        if self.count < 1:
            raise ValueError('MeanTeacher: the models hold no float32 tensor')
        dev = self.pairs[0][1].device
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)     # one copy, once per model
        self.chunk_first = torch.tensor(first, dtype=torch.int64).to(dev)
        self.numel = sum(d.numel() for _, d, _ in self.pairs)
        self._ptrs = [(d, d.data_ptr(), s, s.data_ptr()) for _, d, s in self.pairs]

    def _valid(self):
        return all(d.data_ptr() == dp and s.data_ptr() == sp for d, dp, s, sp in self._ptrs)

    @property
    def models(self):
        """(cnn, siamese): the teacher's modules -- ``ATTEvaluator(*teacher.models)`` evaluates and clusters with it."""
        return self.cnn, self.siamese

    def factors(self):
        """(a, 1 - a) of the next update as the float32 values the kernel receives."""
        a = ema_alpha(self.step, self.alpha)
        return C.c_float(a).value, C.c_float(1.0 - a).value

    def update(self):
        from grl_amd import engine
        if not self._valid():                              # a tensor's storage moved (.to(), a new Parameter): a new table
            self._build()
        a, oma = self.factors()
        _call('grl_ema_update', ptr(self.table), ptr(self.chunk_first), self.count, C.c_float(a), C.c_float(oma))
        engine.touch_state(self.cnn)
        engine.touch_state(self.siamese)
        self.step += 1

    def state_dict(self):
        """{'cnn': {'state_dict': ..}, 'siamese': {'state_dict': ..}, 'step', 'alpha'}: each module under the key its
        checkpoint file has (``checkpoint['state_dict']``)."""
        return {'cnn': {'state_dict': self.cnn.state_dict()}, 'siamese': {'state_dict': self.siamese.state_dict()},
                'step': self.step, 'alpha': self.alpha}

    def load_state_dict(self, state):
        from grl_amd import engine
        self.cnn.load_state_dict(state['cnn']['state_dict'])
        self.siamese.load_state_dict(state['siamese']['state_dict'])
        self.step, self.alpha = int(state['step']), float(state['alpha'])
        engine.touch_state(self.cnn)
        engine.touch_state(self.siamese)

    def rows(self, clips, siamese_model_uncorr=None):
        """The teacher's three row sets for ``SEQTrainer._forward``'s identity criteria, from ONE eval forward of the clip
        tensor the student sees, under ``torch.no_grad()``:
          ('uncorr', 'clip')   x_uncorr in ``siamese_model_uncorr``'s probe-then-gallery order (that head has no parameter on
                               the identity path: the reorder alone)
          ('corr', 'frame')    x_corr.reshape(B T, -1)
          ('corr', 'clip')     the teacher Siamese's eval-mode forward(x_corr)[1]
        gathered in rank order under GRL_DP_GLOBAL_HEADS, as the student's outputs."""
        with torch.no_grad():
            x_uncorr, x_corr = self.cnn(clips)
            if grl_dist.global_heads():
                x_uncorr, x_corr = grl_dist.gather_global(x_uncorr), grl_dist.gather_global(x_corr)
            b, t = x_corr.size(0), x_corr.size(1)
            xv = x_uncorr.contiguous().view(b // 2, 2, -1)
            return {('uncorr', 'clip'): torch.cat((xv[:, 0], xv[:, 1])).contiguous(),
                    ('corr', 'frame'): x_corr.reshape(b * t, -1),
                    ('corr', 'clip'): self.siamese(x_corr)[1]}


class MeanTeacherMixin(object):
    """The teacher's part of a trainer's step, in front of any SEQTrainer in the method resolution order
    (``MeanTeacherSEQTrainer``, ``MeanTeacherHybridSEQTrainer``, ``MeanTeacherCameraSEQTrainer``): the teacher's rows fetched
    before the base's forward, the identity criteria called with ``teacher=`` / ``soft_weight=`` next to what the base hands
    them, the soft triplet term, and the teacher's update hooked behind ``optimizer.step()``.  ``GraphedTrainStep`` refuses
    every trainer that carries it.  With ``ins_hard_weight`` / ``ins_soft_weight`` != 0 the triplet term is followed by an owned
    ``InstanceContrastLoss`` on the same rows; with the defaults 0 nothing is called."""

    ins_hard_weight = 0.0
    ins_soft_weight = 0.0

    soft_class = None               # the criterion class both identity criteria must be; a trainer sets it

    def __init__(self, cnn_model, siamese_model, siamese_model_uncorr, criterion_veri, criterion_corr, criterion_uncorr, logdir,
                 teacher=None, soft_weight=0.5, tri_soft_weight=0.0, ins_hard_weight=0.0, ins_soft_weight=0.0, ins_tau=0.1,
                 ins_teacher_tau=None):
        """The base trainer's constructor behind the checks, each a ValueError naming the trainer and the argument, before
        anything is stored."""
        who, soft_class = type(self).__name__, self.soft_class
        for name, crit in (('criterion_corr', criterion_corr), ('criterion_uncorr', criterion_uncorr)):
            if not isinstance(crit, soft_class):
                raise ValueError('%s: %s must be a %s (got %s)' % (who, name, soft_class.__name__, type(crit).__name__))
        if criterion_corr is criterion_uncorr:
            raise ValueError('%s: criterion_corr and criterion_uncorr must be two objects (the criterion '
                             "decides which branch's teacher rows it is given)" % who)
        if not isinstance(teacher, MeanTeacher):
            raise ValueError('%s: teacher must be a MeanTeacher (got %s)' % (who, type(teacher).__name__))
        if not 0.0 <= float(soft_weight) <= 1.0:
            raise ValueError('%s: soft_weight must be in [0, 1] (got %r)' % (who, soft_weight))
        if not 0.0 <= float(tri_soft_weight) <= 1.0:
            raise ValueError('%s: tri_soft_weight must be in [0, 1] (got %r)' % (who, tri_soft_weight))
        check_ins_weights(ins_hard_weight, ins_soft_weight, who=who, names=('ins_hard_weight', 'ins_soft_weight'),
                          allow_both_zero=True)
        check_temperature('ins_tau', ins_tau, who=who)
        if ins_teacher_tau is not None:
            check_temperature('ins_teacher_tau', ins_teacher_tau, who=who)
        super(MeanTeacherMixin, self).__init__(cnn_model, siamese_model, siamese_model_uncorr, criterion_veri, criterion_corr,
                                               criterion_uncorr, logdir)
        self.teacher = teacher
        self.soft_weight = float(soft_weight)
        self.tri_soft_weight = float(tri_soft_weight)
        self.criterion_soft_triplet = SoftTripletLoss()
        self.ins_hard_weight = float(ins_hard_weight)
        self.ins_soft_weight = float(ins_soft_weight)
        self.criterion_ins = InstanceContrastLoss(tau=ins_tau, teacher_tau=ins_teacher_tau)
        self._teacher_rows = None

    def _forward(self, inputs, targets, i, epoch):
        """The teacher's rows first, on the launch stream and BEFORE the base forks its side stream, which reads them (the
        constraint of ``HybridSEQTrainer._parse_data``).  Both weights 0: no teacher pass, the base's launches."""
        need = (self.soft_weight != 0.0 or self.tri_soft_weight != 0.0 or self.ins_hard_weight != 0.0
                or self.ins_soft_weight != 0.0)
        self._teacher_rows = self.teacher.rows(inputs[0], self.siamese_model_uncorr) if need else None
        return super(MeanTeacherMixin, self)._forward(inputs, targets, i, epoch)

    def _id_loss(self, criterion, feats, targets, rows):
        if self._teacher_rows is None:
            return criterion(feats, targets, teacher=None, soft_weight=0.0, **self._id_extra(rows))
        branch = 'uncorr' if criterion is self.criterion_uncorr else 'corr'
        return criterion(feats, targets, teacher=self._teacher_rows[(branch, rows)], soft_weight=self.soft_weight,
                         **self._id_extra(rows))

    def _tri_loss(self, feats, target):
        if self.tri_soft_weight == 0.0:
            tri = super(MeanTeacherMixin, self)._tri_loss(feats, target)
        else:
            tri = self.criterion_soft_triplet(feats, target, teacher=self._teacher_rows[('corr', 'clip')],
                                              soft_weight=self.tri_soft_weight).mean()
        if self.ins_hard_weight == 0.0 and self.ins_soft_weight == 0.0:
            return tri
        return tri + self.criterion_ins(feats, target, teacher=self._teacher_rows[('corr', 'clip')],
                                        hard_weight=self.ins_hard_weight, soft_weight=self.ins_soft_weight).mean()

    def train(self, epoch, data_loader, optimizer1):
        hook = optimizer1.register_step_post_hook(lambda *_: self.teacher.update())
        try:
            super(MeanTeacherMixin, self).train(epoch, data_loader, optimizer1)
        finally:
            hook.remove()
            self._teacher_rows = None


class MeanTeacherSEQTrainer(MeanTeacherMixin, SEQTrainer):
    """SEQTrainer's constructor plus ``teacher=`` (a ``MeanTeacher`` over ``cnn_model`` and ``siamese_model``),
    ``soft_weight=`` and ``tri_soft_weight=``; ``criterion_corr`` and ``criterion_uncorr`` are two ``SoftClusterMemoryLoss``
    and are called as ``criterion(feats, targets, teacher=rows, soft_weight=soft_weight)``.  With ``tri_soft_weight`` != 0 the
    batch-hard triplet term is an owned ``SoftTripletLoss`` against the teacher's ('corr', 'clip') rows; with
    the default 0 it is SEQTrainer's.  With ``ins_hard_weight`` / ``ins_soft_weight`` != 0 (temperatures ``ins_tau``,
    ``ins_teacher_tau``; None: ``ins_tau``) an owned ``InstanceContrastLoss`` on the same rows is added to it.
    ``train`` updates the teacher behind every optimizer step."""

    soft_class = SoftClusterMemoryLoss


class MeanTeacherHybridSEQTrainer(MeanTeacherMixin, HybridSEQTrainer):
    """``HybridSEQTrainer`` with a mean teacher: ``MeanTeacherSEQTrainer``'s extra arguments;
    ``criterion_corr`` and ``criterion_uncorr`` are two ``SoftHybridMemoryLoss`` and are called as
    ``criterion(feats, targets, index=index, teacher=rows, soft_weight=soft_weight)``.  Batches carry their instance indices
    as ``HybridSEQTrainer``'s do."""

    soft_class = SoftHybridMemoryLoss


class MeanTeacherCameraSEQTrainer(MeanTeacherMixin, CameraSEQTrainer):
    """``CameraSEQTrainer`` with a mean teacher: ``MeanTeacherSEQTrainer``'s extra arguments;
    ``criterion_corr`` and ``criterion_uncorr`` are two ``SoftProxyMemoryLoss`` and are called as
    ``criterion(feats, targets, cams=cams, teacher=rows, soft_weight=soft_weight)``."""

    soft_class = SoftProxyMemoryLoss
