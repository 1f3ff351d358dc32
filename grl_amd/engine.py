"""Host-side orchestration of the GRL hot path on MI355X.

Python here only owns device memory (torch tensors), weight packing caches and
the launch order; every FLOP is issued through the C ABI in include/grl_hip.h
(libgrl_hip.so, hand-written HIP for gfx950).  Activations are channels-last
row-major matrices [N*H*W][C] from the stem to the TRL head.

Reference call sites (relative to /root/reference):
  grl_forward             reid/models/grl_model.py:211-228
    trunk                 reid/models/resnets1.py:73-93,101-109
    GCE                   reid/models/basebranch.py:52-68
    TRL                   reid/models/grl_model.py:131-180
  siamese_self_attention  reid/models/Siamese.py:79-106
  extract_features        reid/evaluator/attevaluator.py:100-112
  cosin_dist/pairwise     reid/evaluator/attevaluator.py:33-46
"""
import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import GrlGemm, GrlBneckTail, GrlBneckTailF32, EPI_AFFINE, EPI_NEGDOT, EPI_EUCLID, EPI_SQDIFF, check, ptr, require_device

import contextlib
import numbers
import os

from ._lib import MATH_F32, MATH_BF16, MATH_BF16X3, MATH_BF16S, MATH_MXFP8

_MATH_NAMES = {'f32': MATH_F32, 'bf16': MATH_BF16, 'bf16x3': MATH_BF16X3, 'bf16s': MATH_BF16S}
# Multiplier datapath of the conv / linear GEMMs (accumulation is always fp32):
#   'f32'    exact fp32 MFMA, the default and the mode every parity claim is made in;
#   'bf16x3' split-bf16 (hi*hi + hi*lo + lo*hi), ~2^-16 relative per product;
#   'bf16'   operands rounded to bf16 while staging, activations still fp32 in HBM;
#   'bf16s'  bf16 STORAGE: activations and weights are bf16 in HBM from the stem to the TRL
#            memo (BASELINE configs[2] pipeline); per-clip vectors and the tail stay fp32.
# The evaluator distance matrices always use 'f32' (bit-exact ranking contract).
#
# EXPERIMENTAL, not a user mode: 'mxfp8' = the 'bf16s' pipeline with its generic conv / linear GEMMs on MX-FP8 operands
# (e4m3 elements, one power-of-two scale per 32 k: include/grl_hip.h "MX-FP8 datapath"; the fused bf16 kernels, the
# fp32 per-clip linears and the tail stay as in 'bf16s').  It is measured SLOWER than 'bf16s' (EXPERIMENTS.md,
# 'MX-FP8 eval datapath') and less accurate, so set_math / math_mode / GRL_MATH do not accept it; the tests and
# tools/mxfp8_rate.py reach it through experimental_math('mxfp8').  Eval only: train_engine refuses it.
_EXPERIMENTAL_MATH = {'mxfp8': MATH_MXFP8}
_math = [_MATH_NAMES[os.environ.get('GRL_MATH', 'f32')]]


def set_math(name):
    _math[0] = _MATH_NAMES[name]


def get_math():
    return {v: k for k, v in list(_MATH_NAMES.items()) + list(_EXPERIMENTAL_MATH.items())}[_math[0]]


@contextlib.contextmanager
def experimental_math(name):
    """Run the enclosed eval calls on an experimental datapath (only 'mxfp8' today; see above) -- for measurement
    and tests, not a supported mode."""
    old = _math[0]
    _math[0] = _EXPERIMENTAL_MATH[name]
    try:
        yield
    finally:
        _math[0] = old


@contextlib.contextmanager
def math_mode(name):
    old = _math[0]
    set_math(name)
    try:
        yield
    finally:
        _math[0] = old


FUSE_TRL_SQDIFF = True     # TRL step: (ReLU(f1) - f2)^2 GAP inside the f1 GEMM epilogue (A/B switch for tools/)
PIX = 128            # 16 x 8 feature map of layer4 (basebranch.py:59 hard-codes it)


# ----------------------------------------------------------------------------
# thin launch wrappers
# ----------------------------------------------------------------------------
def _new(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _newl(shape, like):
    return torch.empty(shape, dtype=like.dtype, device=like.device)


def _k(name, t):
    """Entry point for tensor ``t``'s storage type: the bf16 twin (train_bf16.hip / pointwise_bf16.hip) or the fp32 one."""
    return name + '_bf16' if t.dtype == torch.bfloat16 else name


# Raw uint8 clips are normalised on the device with the constants of the reference's loaders
# (reid/data/dataloader.py:20,51: ToTensor + Normalize(mean, std)) -- inside the stem in eval
# mode, by grl_normalize_u8 in train mode.  SURVEY.md 8(f) rank 4.
INPUT_MEAN = (0.485, 0.456, 0.406)
INPUT_STD = (0.229, 0.224, 0.225)
_mean_std = {}


def input_mean_std(dev):
    t = _mean_std.get(dev)
    if t is None:
        t = _mean_std[dev] = torch.tensor(INPUT_MEAN + INPUT_STD, dtype=torch.float32, device=dev)
    return t


def normalize_u8(x):
    """uint8 [..., 3, H, W] -> float32, (x/255 - mean)/std per channel (bit-identical to the host
    ToTensor + Normalize of seqtransforms.py:190,212-213)."""
    require_device(x, 'clips', allow_u8=True)
    if x.dtype != torch.uint8:
        return x
    x = x.contiguous()
    y = _new(x.shape, x)
    plane = x.shape[-1] * x.shape[-2]
    _call('grl_normalize_u8', ptr(x), ptr(input_mean_std(x.device)), ptr(y), x.numel() // (3 * plane), plane)
    return y


_resize_tables = {}


def rect_scale_u8(x, height=256, width=128):
    """RectScale(height, width) of the reference's loaders (seqtransforms.py:30-47, dataloader.py:53,68)
    on the device: uint8 frames [..., 3, Hin, Win] -> [..., 3, height, width], bit-identical to PIL's
    BILINEAR resize (frames that already have the size are returned as they are, as upstream)."""
    require_device(x, 'frames', allow_u8=True)
    if x.dtype != torch.uint8:
        raise ValueError('rect_scale_u8 expects raw uint8 frames')
    hin, win = x.shape[-2:]
    if (hin, win) == (height, width):
        return x
    key = (hin, win, height, width, x.device)
    tabs = _resize_tables.get(key)
    if tabs is None:
        from .reid.data.augment import pil_bilinear_coeffs
        bh, ch = pil_bilinear_coeffs(win, width)
        bv, cv = pil_bilinear_coeffs(hin, height)
        tabs = _resize_tables[key] = tuple(torch.from_numpy(t).contiguous().to(x.device) for t in (bh, ch, bv, cv))
    bh, ch, bv, cv = tabs
    x = x.contiguous()
    y = torch.empty(x.shape[:-2] + (height, width), dtype=torch.uint8, device=x.device)
    _call('grl_resize_bilinear_u8', ptr(x), ptr(y), ptr(bh), ptr(ch), ch.shape[1], ptr(bv), ptr(cv), cv.shape[1],
          x.numel() // (hin * win), hin, win, height, width)
    return y


def augment_normalize_u8(clips, params):
    """Training augmentation on the device: uint8 clips [B,T,3,H,W] + the host-drawn decisions
    (int32 [B, 1 + 8T], grl_amd.reid.data.augment) -> float32 clips, flipped / erased / normalised
    exactly as the reference's PIL transforms would (seqtransforms.py:92-190, dataloader.py:51-57)."""
    require_device(clips, 'clips', allow_u8=True)
    if clips.dtype != torch.uint8 or clips.dim() != 5 or clips.shape[2] != 3:
        raise ValueError('augment_normalize_u8 expects uint8 clips [B,T,3,H,W]')
    b, t, _, h, w = clips.shape
    params = params.to(device=clips.device, dtype=torch.int32).contiguous()
    if tuple(params.shape) != (b, 1 + 8 * t):
        raise ValueError('augmentation parameters must be [B, 1 + 8*T] (got %s)' % (tuple(params.shape),))
    clips = clips.contiguous()
    y = _new(clips.shape, clips)
    _call('grl_augment_normalize_u8', ptr(clips), ptr(params), ptr(input_mean_std(clips.device)), ptr(y), b, t, h, w)
    return y


FUSE_BNECK = os.environ.get('GRL_FUSE_BNECK', '1') != '0'       # A/B and tests: 0 = one launch per convolution
FUSE_STEM_POOL = os.environ.get('GRL_FUSE_STEM_POOL', '1') != '0'   # A/B and tests: 0 = stem and max-pool as two launches (bf16 storage)
FUSE_STEM_POOL_F32 = os.environ.get('GRL_FUSE_STEM_POOL_F32', '1') != '0'   # ... the exact-fp32 path (round 5)
FUSE_DOWN = os.environ.get('GRL_FUSE_DOWN', '1') != '0'         # A/B and tests: 0 = the downsample conv as its own launch
SLAB_CHECK = False  # tests only: poison every statistics slab and verify that the GEMM wrote all of it
SPLITK = True       # tests / A-B only: False = never hand the library split-K scratch (one workgroup per tile walks K)


def gemm(a, w, y, M, N, K, lda=0, ldw=None, ldy=None, scale=None, shift=None, res=None,
         ldres=0, gbias=None, rows_per_group=0, rowscale=None, relu=False,
         epilogue=EPI_AFFINE, rnorm=None, cnorm=None, stats=None, conv=None, math=None, out_f32=False,
         kblock=False, res_rows=0, res_gstride=0, bn=None):
    """Y[M][N] = epilogue(A . W^T) through grl_conv_gemm_f32.  ``conv`` is
    (H, W, C, Ho, Wo, kh, kw, stride, pad) for an implicit-GEMM convolution.
    ``stats=True`` allocates and returns the per-channel partial-sum slab
    (train-mode BatchNorm) as ``(y, slab)``."""
    want_stats = stats is True
    if want_stats:
        stats = None
    # one positional constructor call in the struct's field order (include/grl_hip.h GrlGemm / _lib.GrlGemm) instead of ~30
    # attribute stores: this wrapper runs ~220 times per training step, which is host-bound in bf16 storage (round 6)
    cv = (1,) + tuple(conv) if conv is not None else (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    bnp = tuple(ptr(t) for t in bn) if bn is not None else ()        # BatchNorm-backward reduce in the epilogue (GrlGemm.bn_z; with stats=True)
    d = GrlGemm(ptr(a), ptr(w), ptr(y), ptr(scale), ptr(shift), ptr(res), ptr(gbias), ptr(rowscale), ptr(rnorm), ptr(cnorm),
                ptr(stats), M, N, K, lda or K, ldw or K, ldy or N, ldres or N, rows_per_group, 1 if relu else 0, epilogue,
                cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7], cv[8], cv[9],
                (MATH_F32 if _math[0] in (MATH_BF16S, MATH_MXFP8) else _math[0]) if math is None else math, 1 if out_f32 else 0,
                res_rows, res_gstride, 1 if kblock else 0, None, 0, *bnp)
    lib = _lib.load()
    if d.math == MATH_MXFP8:                  # the activations' MX image (include/grl_hip.h: required scratch)
        need = lib.grl_conv_gemm_f32_workspace_floats(C.byref(d))
        if need > 0:
            ws = torch.empty(need, dtype=torch.float32, device=y.device)
            d.splitk_ws, d.splitk_ws_floats = ptr(ws), need
    elif SPLITK and kblock and conv is None and M <= 256 and K > 512:      # skinny K-blocked GEMM: split-K scratch (include/grl_hip.h)
        need = lib.grl_conv_gemm_f32_workspace_floats(C.byref(d))
        if need > 0:
            ws = torch.empty(need, dtype=torch.float32, device=y.device)
            d.splitk_ws, d.splitk_ws_floats = ptr(ws), need
    if want_stats:
        rows = lib.grl_conv_gemm_f32_stat_rows(C.byref(d))
        # (`rows` is the row count of the kernel that takes THIS launch -- two per 256-row tile of the bf16 256 x 256 kernel,
        #  one per tile row of the 128-row family -- and every one of them is written, ragged last tiles included: no fill.
        #  Rounds 2-4 zero-filled the bf16-storage slabs defensively: 79 fill launches per training step.  SLAB_CHECK
        #  (tests): poison the slab and verify after the launch that nothing of the poison is left.)
        slab = torch.empty((rows, 2, N), dtype=torch.float32, device=y.device)
        if SLAB_CHECK:
            slab.fill_(float('nan'))
        d.stats = ptr(slab)
        check(lib.grl_conv_gemm_f32(C.byref(d), _lib.stream()), 'grl_conv_gemm_f32')
        if SLAB_CHECK and bool(torch.isnan(slab).any()):
            raise AssertionError('statistics slab of gemm %s math %d conv %s: %d of %d rows not written' % (
                (M, N, K), d.math, conv, int(torch.isnan(slab).any(dim=2).any(dim=1).sum()), rows))
        if _DEBUG_SYNC:
            _debug_sync('gemm+stats %s math %d conv %s' % ((M, N, K), d.math, conv))
        return y, slab
    check(lib.grl_conv_gemm_f32(C.byref(d), _lib.stream()), 'grl_conv_gemm_f32')
    if _DEBUG_SYNC:
        _debug_sync('gemm %s math %d conv %s' % ((M, N, K), d.math, conv))
    return y


def gemm_group(calls):
    """Several dense GEMMs of ONE shape in one launch where the library can group them (grl_conv_gemm_f32_group;
    bit-identical to ``gemm(**c)`` for every c in order, which is also what it falls back to).  ``calls``: list of
    dicts with the plain-affine keyword subset of :func:`gemm` (a, w, y, M, N, K, scale, shift, res, relu, math, ld*)."""
    n = len(calls)
    arr = (GrlGemm * n)()
    for d, c in zip(arr, calls):
        d.a, d.w, d.y = ptr(c['a']), ptr(c['w']), ptr(c['y'])
        d.scale, d.shift, d.res = ptr(c.get('scale')), ptr(c.get('shift')), ptr(c.get('res'))
        d.M, d.N, d.K = c['M'], c['N'], c['K']
        d.lda = c.get('lda') or d.K
        d.ldw = c.get('ldw') or d.K
        d.ldy = c.get('ldy') or d.N
        d.ldres = c.get('ldres') or d.N
        d.relu = 1 if c.get('relu') else 0
        d.epilogue = EPI_AFFINE
        m = c.get('math')
        d.math = (MATH_F32 if _math[0] in (MATH_BF16S, MATH_MXFP8) else _math[0]) if m is None else m
    check(_lib.load().grl_conv_gemm_f32_group(arr, n, _lib.stream()), 'grl_conv_gemm_f32_group')
    if _DEBUG_SYNC:
        _debug_sync('gemm_group x%d %s' % (n, (calls[0]['M'], calls[0]['N'], calls[0]['K'])))
    return [c['y'] for c in calls]


_DEBUG_SYNC = bool(os.environ.get('GRL_DEBUG_SYNC'))      # debugging only: name every launch on stderr and wait for it


def _debug_sync(name):
    import sys
    sys.stderr.write('[grl] %s\n' % name)
    sys.stderr.flush()
    torch.cuda.synchronize()


_fns = {}


def _kb():
    """The per-clip linears of the eval path (global descriptor, its bias term, the Siamese Q|K projection: M = clips or
    frames, K = 1024..2048) accumulate K-BLOCKED in the exact-fp32 datapath: their 512-k segments then run as separate
    workgroups (GrlGemm.splitk_ws) instead of one workgroup per tile walking all of K -- 55 -> ~15 us each -- and the
    result does not depend on whether the library splits (M <= 256) or not: a clip's row stays batch-independent."""
    return _math[0] in (MATH_F32, MATH_BF16S, MATH_MXFP8)


def _call(name, *args):
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(_lib.load(), name)
    rc = fn(*args, _lib.stream())
    if rc:
        check(rc, name)
    if _DEBUG_SYNC:
        _debug_sync(name)


# ----------------------------------------------------------------------------
# packed parameters
# ----------------------------------------------------------------------------
class _Conv(object):
    """A conv (or linear) with its eval-folded affine."""
    __slots__ = ('w', 'N', 'K', 'ldw', 'scale', 'shift', 'k', 'stride', 'cin', '_wb', '_wperm', '_wmx')

    def wb(self):
        """bf16 copy of the packed weight (bf16-storage pipeline), made on first use."""
        if getattr(self, '_wb', None) is None:
            w = self.w.contiguous()
            self._wb = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
            _call('grl_cast_bf16', ptr(w), ptr(self._wb), w.numel())
        return self._wb

    def wmx(self, K=None):
        """MX-FP8 image of the packed weight's first ``K`` (default all) columns (grl_mx_pack_weights; the
        'mxfp8' datapath), made on first use.  The plan is rebuilt when the module's state changes, so is this."""
        K = K or self.K
        if getattr(self, '_wmx', None) is None or self._wmx[0] != K:
            w = self.w.contiguous()
            ldw = w.shape[1]
            img = torch.empty(_lib.load().grl_mx_image_bytes(self.N, K), dtype=torch.uint8, device=w.device)
            _call('grl_mx_pack_weights', ptr(w), self.N, K, ldw, ptr(img))
            self._wmx = (K, img)
        return self._wmx[1]

    def wperm(self):
        """bf16 copy of a 1x1 weight [N][K] in the k order the chained MFMA of grl_bottleneck_tail_bf16 consumes
        (grl_bneck_perm32), made on first use."""
        if getattr(self, '_wperm', None) is None:
            w = self.w.contiguous()
            self._wperm = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
            _call('grl_bneck_perm32', ptr(w), 0, ptr(self._wperm), w.shape[0], w.shape[1])
        return self._wperm


def _state_key(module):
    """Identity of a module's state for the packed-plan caches: (pointer, torch version counter)
    of every parameter / buffer plus the module's train-forward generation.  The train-mode
    kernels update BatchNorm running statistics through raw device pointers, which torch's
    version counters never see -- ``touch_state`` (called by every train-mode forward) makes those
    updates visible here, so eval -> train forward under no_grad -> eval re-folds the BatchNorms."""
    return (getattr(module, '_grl_generation', 0),) + tuple(
        (t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))


def touch_state(module):
    """Mark ``module``'s buffers as changed behind torch's back (see ``_state_key``)."""
    module._grl_generation = getattr(module, '_grl_generation', 0) + 1


class EvalPlan(object):
    """Device-side packing of a model's parameters for the eval forward:
    3x3 weights re-laid tap-major, BatchNorm folded to scale/shift, Q|K weights
    concatenated.  Rebuilt whenever a parameter/buffer changes (version
    counters), so load_state_dict / optimizer steps are picked up."""

    def __init__(self, module):
        self.key = _state_key(module)
        self.dev = next(module.parameters()).device

    # -- helpers ---------------------------------------------------------------
    def fold(self, bn=None, bias=None, n=None):
        """(scale, shift) of eval BN (optionally after a biased layer)."""
        n = n if n is not None else (bn.num_features if bn is not None else bias.numel())
        scale = torch.empty(n, dtype=torch.float32, device=self.dev)
        shift = torch.empty(n, dtype=torch.float32, device=self.dev)
        if bn is not None:
            _call('grl_bn_fold', ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                  ptr(bn.running_var), ptr(bias), C.c_float(bn.eps), ptr(scale), ptr(shift), n)
        else:
            _call('grl_bn_fold', None, None, None, None, ptr(bias), C.c_float(0.0), ptr(scale),
                  ptr(shift), n)
        return scale, shift

    def conv(self, conv, bn=None):
        c = _Conv()
        c._wb = None
        c._wperm = None
        c._wmx = None
        w = conv.weight.detach()
        c.N, c.cin = w.shape[0], w.shape[1]
        c.k = w.shape[2] if w.dim() == 4 else 1
        c.stride = conv.stride[0] if hasattr(conv, 'stride') else 1
        if c.k == 1:
            c.w = w.contiguous().view(c.N, c.cin)
        else:
            c.w = torch.empty(c.N, c.k * c.k * c.cin, dtype=torch.float32, device=self.dev)
            wc = w.contiguous()          # must outlive the launch below
            _call('grl_pack_conv_weight', ptr(wc), ptr(c.w), c.N, c.cin, c.k, c.k)
        c.K = c.w.shape[1]
        c.ldw = c.K
        bias = getattr(conv, 'bias', None)
        if bn is not None:
            c.scale, c.shift = self.fold(bn, bias.detach() if bias is not None else None)
        elif bias is not None:
            c.scale, c.shift = None, bias.detach()
        else:
            c.scale, c.shift = None, None
        return c


class GrlEvalPlan(EvalPlan):
    def __init__(self, model):
        super().__init__(model)
        bb = model.backbone
        base = bb.base
        self.stem_w = base[0].weight.detach().contiguous()
        self.stem_wp = torch.empty(64 * 164, dtype=torch.float32, device=self.dev)
        _call('grl_stem_pack_weight', ptr(self.stem_w), ptr(self.stem_wp))
        self.stem_wpb = torch.empty(64 * 184, dtype=torch.bfloat16, device=self.dev)
        _call('grl_stem_pack_weight_bf16', ptr(self.stem_w), ptr(self.stem_wpb))
        self.stem_wq = torch.empty(64 * 168, dtype=torch.float32, device=self.dev)
        _call('grl_stem_pack_weight_pool', ptr(self.stem_w), ptr(self.stem_wq))
        self.stem_scale, self.stem_shift = self.fold(base[1])
        self.blocks = []
        for li in (4, 5, 6, 7):
            for blk in base[li]:
                e = dict(c1=self.conv(blk.conv1, blk.bn1), c2=self.conv(blk.conv2, blk.bn2),
                         c3=self.conv(blk.conv3, blk.bn3), down=None, stride=blk.stride)
                if blk.downsample is not None:
                    e['down'] = self.conv(blk.downsample[0], blk.downsample[1])
                self.blocks.append(e)
        # GCE (basebranch.py:38-50)
        self.glo_fc = self.conv(bb.glo_fc[0], bb.glo_fc[1])
        self.corr0 = self.conv(bb.corr_atte[0], bb.corr_atte[1])        # [1024][3072]
        self.corr2 = self.conv(bb.corr_atte[2], bb.corr_atte[3])
        self.corr5_w = bb.corr_atte[5].weight.detach().contiguous().view(-1)
        self.corr6_scale, self.corr6_shift = self.fold(bb.corr_atte[6])
        # TRL (grl_model.py:93-128)
        trl = model.temporal_learning_block
        self.dirs = []
        for f1, f2, mlp, memo in (
                (trl.forward_f1, trl.forward_f2, trl.channel_atte_foreward_corr, trl.uncorr_memo_forward),
                (trl.backward_f1, trl.backward_f2, trl.channel_atte_backward_corr, trl.uncorr_memo_backward)):
            self.dirs.append(dict(
                f1=self.conv(f1[0]), f2=self.conv(f2[0]),
                w1=mlp[0].weight.detach().contiguous(),
                w2t=mlp[2].weight.detach().t().contiguous(),
                c1=self.conv(memo.conv1, memo.bn1), c2=self.conv(memo.conv2, memo.bn2),
                c3=self.conv(memo.conv3, memo.bn3)))
        self.corr_bn = self.fold(model.corr_bn)
        self.uncorr_bn = self.fold(model.uncorr_bn)


class SiameseEvalPlan(EvalPlan):
    def __init__(self, siam):
        super().__init__(siam)
        self.D = siam.featQ.out_features
        self.wqk = torch.cat((siam.featQ.weight.detach(), siam.featK.weight.detach()), 0).contiguous()
        sq, hq = self.fold(siam.featQ_bn, siam.featQ.bias.detach())
        sk, hk = self.fold(siam.featK_bn, siam.featK.bias.detach())
        self.scale = torch.cat((sq, sk)).contiguous()
        self.shift = torch.cat((hq, hk)).contiguous()


_plans = weakref.WeakKeyDictionary()


def _plan(module, cls):
    """Cached plan of class ``cls`` for ``module`` (a module may own several kinds: a Siamese
    has an attention plan and a verification-head plan); rebuilt when its state changes."""
    per = _plans.get(module)
    if per is None:
        per = {}
        _plans[module] = per
    p = per.get(cls)
    if p is None or p.key != _state_key(module):
        p = cls(module)
        per[cls] = p
    return p


# ----------------------------------------------------------------------------
# eval forward
# ----------------------------------------------------------------------------
def _newb(shape, like):
    return torch.empty(shape, dtype=torch.bfloat16, device=like.device)


FUSE_C64 = os.environ.get('GRL_CONV3X3_C64', '1') != '0'        # A/B and tests: 0 = layer 1's 3x3 convs on the generic kernel


def conv3x3_c64_bf16(x, c, n_img, H, W, relu=True):
    """Layer 1's 3x3 / stride 1, 64 -> 64 channels, W == 32 (resnets1.py:79-81): weights LDS-resident, each input pixel
    staged once per tile (grl_conv3x3_c64_bf16)."""
    y = _newb((n_img * H * W, 64), x)
    _call('grl_conv3x3_c64_bf16', ptr(x), ptr(c.wb()), ptr(c.scale), ptr(c.shift), ptr(y), n_img, H, W, 1 if relu else 0)
    return y


def _gw(c, x, dp, K=None):
    """(weight, math) of a generic conv / linear GEMM over the activation ``x``.  fp32 storage: the packed fp32 weight on
    the mode's multiplier datapath (math None: gemm()'s default).  bf16 storage: the bf16 copy on MATH_BF16S or, with
    ``dp`` = MATH_MXFP8, the MX-FP8 image of the weight's first ``K`` (default all) columns."""
    if x.dtype != torch.bfloat16:
        return c.w, None
    return (c.wmx(K), MATH_MXFP8) if dp == MATH_MXFP8 else (c.wb(), MATH_BF16S)


def _conv_layer(x, c, n_img, H, W, stride=1, relu=True, res=None, dp=MATH_BF16S, **kw):
    """x: [n_img*H*W][cin] channels-last, fp32 or bf16 storage: the output follows it (``dp``: see _gw).
    Returns (y, Ho, Wo)."""
    if (x.dtype == torch.bfloat16 and FUSE_C64 and c.k == 3 and stride == 1 and c.cin == 64 and c.N == 64 and W == 32
            and H % 8 == 0 and res is None and not kw and n_img * H * W * 128 < (1 << 32)):          # (32-bit byte offsets inside that kernel)
        return conv3x3_c64_bf16(x, c, n_img, H, W, relu), H, W
    wt, m = _gw(c, x, dp)
    if c.k == 1 and stride == 1:
        M = n_img * H * W
        y = _newl((M, c.N), x)
        gemm(x, wt, y, M, c.N, c.K, ldw=c.ldw, scale=c.scale, shift=c.shift, res=res, relu=relu, math=m, **kw)
        return y, H, W
    pad = c.k // 2
    Ho = (H + 2 * pad - c.k) // stride + 1
    Wo = (W + 2 * pad - c.k) // stride + 1
    M = n_img * Ho * Wo
    y = _newl((M, c.N), x)
    gemm(x, wt, y, M, c.N, c.K, ldw=c.ldw, scale=c.scale, shift=c.shift, res=res, relu=relu,
         conv=(H, W, c.cin, Ho, Wo, c.k, c.k, stride, pad), math=m, **kw)
    return y, Ho, Wo


def _to_nchw(y, n, H, W):
    return y.view(n, H, W, -1).permute(0, 3, 1, 2)


STAGE_HOOK = None      # bench.py's per-stage timing pass: callable(stage name) at every stage boundary of the eval forward


def _stage(name):
    if STAGE_HOOK is not None:
        STAGE_HOOK(name)


def _stem_pool_ok(x, n):
    """what grl_stem_pool_{f32,bf16} require beyond the frame geometry (one grid row per frame; 2-byte loads of u8
    rows, 8-byte loads of fp32 rows): otherwise the two-launch stem + max-pool path takes the batch"""
    return n <= 65535 and x.data_ptr() % (2 if x.dtype == torch.uint8 else 8) == 0


FUSE_TAIL_L23 = os.environ.get('GRL_FUSE_TAIL_L23', '0') != '0'   # the layer 2 -> 3 tail (P 128, 4P 512, P' 256) fused too: measured slower


def _bneck_tail_ok(c3, c1n, M):
    # (the fused kernels address with 32-bit byte offsets: M * C4 * 2 bytes must stay below 4 GiB, else the per-conv
    #  launches -- 64-bit row addressing -- take the block)
    # (round 5: the P' = 256 variant -- layer 2's last block + layer 3's first conv1 -- runs 263 us against 240 us for the
    #  two launches it replaces (tools/bneck_tail_ab.py): a 256-wide second product leaves the kernel neither the
    #  registers (spills in its chunk loop at 16 waves) nor the occupancy; it stays available behind GRL_FUSE_TAIL_L23=1)
    if (c3.K, c3.N, c1n.N) == (128, 512, 256) and not FUSE_TAIL_L23:
        return False
    return (c3.k == 1 and c1n.k == 1 and c1n.K == c3.N and M * c3.N * 2 < (1 << 32) and
            bool(_lib.load().grl_bottleneck_tail_bf16_supported(c3.K, c3.N, c1n.N)))


def _bneck_down_ok(c3, c1n, down, stride):
    """The block's downsample branch (1x1, stride 1: layer 1's first block) can ride in the same launch."""
    return (down is not None and stride == 1 and down.k == 1 and c1n is not None and
            (c3.K, c3.N, c1n.N, down.K) == (64, 256, 64, 64))


def bneck_tail_bf16(t2, c3, res, c1n, M, down=None, x0=None):
    """y = relu(bn3(conv3(t2)) + res) [M][4P] and u = relu(bn1'(conv1'(y))) [M][P'] in one launch
    (grl_bottleneck_tail_bf16; resnets1.py:86-91 + :76-78 of the next block).  c1n None: y only.
    ``down`` / ``x0``: the residual is the block's downsample branch bnd(convd(x0)) (resnets1.py:83-84), computed in
    the same launch instead of being written by one launch and re-read by this one (``res`` is ignored)."""
    d = GrlBneckTail()
    y = _newb((M, c3.N), t2)
    d.t2, d.w3, d.scale3, d.shift3, d.res, d.y = ptr(t2), ptr(c3.wb()), ptr(c3.scale), ptr(c3.shift), ptr(res), ptr(y)
    d.M, d.P, d.C4, d.Pn = M, c3.K, c3.N, 0
    if down is not None:
        d.x0, d.wd, d.scaled, d.shiftd, d.Kd = ptr(x0), ptr(down.wb()), ptr(down.scale), ptr(down.shift), down.K
    u = None
    if c1n is not None:
        u = _newb((M, c1n.N), t2)
        d.w1n, d.scale1n, d.shift1n, d.u, d.Pn = ptr(c1n.wperm()), ptr(c1n.scale), ptr(c1n.shift), ptr(u), c1n.N
    check(_lib.load().grl_bottleneck_tail_bf16(C.byref(d), _lib.stream()), 'grl_bottleneck_tail_bf16')
    if _DEBUG_SYNC:
        _debug_sync('bneck_tail %s' % ((M, c3.K, c3.N, d.Pn),))
    return y, u


def _bneck_tail_f32_ok(c3, c1n, M):
    # (32-bit byte offsets inside the fused kernel: M * C4 * 4 bytes below 4 GiB, else one launch per convolution)
    return (_math[0] == MATH_F32 and c3.k == 1 and c1n.k == 1 and c1n.K == c3.N and M * c3.N * 4 < (1 << 32) and
            bool(_lib.load().grl_bottleneck_tail_f32_supported(c3.K, c3.N, c1n.N)))


def bneck_tail_f32(t2, c3, res, c1n, M):
    """The exact-fp32 twin (grl_bottleneck_tail_f32): bit-identical to conv3 (+res, ReLU) followed by conv1' on
    grl_conv_gemm_f32's one-chain fp32 datapath."""
    d = GrlBneckTailF32()
    y = _new((M, c3.N), t2)
    d.t2, d.w3, d.scale3, d.shift3, d.res, d.y = ptr(t2), ptr(c3.w), ptr(c3.scale), ptr(c3.shift), ptr(res), ptr(y)
    d.M, d.P, d.C4, d.Pn = M, c3.K, c3.N, 0
    u = None
    if c1n is not None:
        u = _new((M, c1n.N), t2)
        d.w1n, d.scale1n, d.shift1n, d.u, d.Pn = ptr(c1n.w), ptr(c1n.scale), ptr(c1n.shift), ptr(u), c1n.N
    check(_lib.load().grl_bottleneck_tail_f32(C.byref(d), _lib.stream()), 'grl_bottleneck_tail_f32')
    if _DEBUG_SYNC:
        _debug_sync('bneck_tail_f32 %s' % ((M, c3.K, c3.N, d.Pn),))
    return y, u


def trunk_eval(plan, x, dp, taps=None):
    """x [n,3,H,W] NCHW, float32 or raw uint8 -> channels-last [n*16*8][2048] (for 256x128 input): fp32, or bf16 on the
    bf16-storage datapaths (``dp`` = MATH_BF16S / MATH_MXFP8)."""
    n, _, H, W = x.shape
    Hs, Ws = H // 2, W // 2
    Hp, Wp = (Hs + 1) // 2, (Ws + 1) // 2
    b16 = dp in (MATH_BF16S, MATH_MXFP8)
    # (the stem's entry points follow the _bf16 suffix rule of _k; its one-launch form, its switch and its packed weights do not)
    fuse_stem, pool, wpool, wstem = ((FUSE_STEM_POOL, 'grl_stem_pool_bf16', plan.stem_wpb, plan.stem_wpb) if b16 else
                                     (FUSE_STEM_POOL_F32, 'grl_stem_pool_f32', plan.stem_wq, plan.stem_wp))
    cur = (_newb if b16 else _new)((n * Hp * Wp, 64), x)
    _stage('stem')
    if fuse_stem and taps is None and W == 128 and H % 4 == 0 and _stem_pool_ok(x, n):
        # stem + max-pool in one launch: the stem map never reaches HBM (grl_stem_pool_f32 / grl_stem_pool_bf16)
        u8 = x.dtype == torch.uint8
        _call(pool, ptr(x), 1 if u8 else 0, ptr(input_mean_std(x.device)) if u8 else None,
              ptr(plan.stem_scale), ptr(plan.stem_shift), ptr(cur), n, H, W, ptr(wpool))
    else:
        stem = _newl((n * Hs * Ws, 64), cur)
        if x.dtype == torch.uint8:           # raw pixels: normalised while the stem stages its patch
            _call(_k('grl_stem_conv7x7_u8', stem), ptr(x), ptr(input_mean_std(x.device)), ptr(plan.stem_w),
                  ptr(plan.stem_scale), ptr(plan.stem_shift), ptr(stem), n, H, W, 1, ptr(wstem))
        else:
            _call(_k('grl_stem_conv7x7', stem), ptr(x), ptr(plan.stem_w), ptr(plan.stem_scale), ptr(plan.stem_shift),
                  ptr(stem), n, H, W, 1, ptr(wstem))
        _call(_k('grl_maxpool3x3s2', stem), ptr(stem), ptr(cur), n, Hs, Ws, 64)
        if taps is not None:
            taps['stem'] = _to_nchw(stem, n, Hs, Ws)
            taps['pool'] = _to_nchw(cur, n, Hp, Wp)
        del stem
    H, W = Hp, Wp
    counts = (3, 4, 6, 3)
    bi = 0
    o1 = None
    for li, nb in enumerate(counts):
        _stage('layer%d' % (li + 1))       # (a fused tail computes the NEXT block's conv1: the first conv1 of layers 2 / 3 is booked here)
        for _ in range(nb):
            e = plan.blocks[bi]
            bi += 1
            s = e['stride']
            if o1 is None:
                o1, _, _ = _conv_layer(cur, e['c1'], n, H, W, dp=dp)
            o2, Ho, Wo = _conv_layer(o1, e['c2'], n, H, W, stride=s, dp=dp)
            nxt = plan.blocks[bi]['c1'] if bi < len(plan.blocks) else None
            M = n * Ho * Wo
            fuse = FUSE_BNECK and nxt is not None and (_bneck_tail_ok if b16 else _bneck_tail_f32_ok)(e['c3'], nxt, M)
            o1 = None
            if fuse and b16 and FUSE_DOWN and _bneck_down_ok(e['c3'], nxt, e['down'], s):
                # layer 1's first block: the downsample branch too -- its 4P-wide output is neither written nor re-read
                cur, o1 = bneck_tail_bf16(o2, e['c3'], None, nxt, M, down=e['down'], x0=cur)
            else:
                res = _conv_layer(cur, e['down'], n, H, W, stride=s, relu=False, dp=dp)[0] if e['down'] is not None else cur
                if fuse:
                    # layers 1-2: conv3 + residual + ReLU AND the next block's conv1 in one launch -- the 4P-wide output is
                    # written once (the next block's residual) and never re-read (fuse_bf16.hip; fuse_f32.hip: bit-identical
                    # to the two GEMM launches)
                    cur, o1 = (bneck_tail_bf16 if b16 else bneck_tail_f32)(o2, e['c3'], res, nxt, M)
                else:
                    cur, _, _ = _conv_layer(o2, e['c3'], n, Ho, Wo, res=res, dp=dp)
            H, W = Ho, Wo
        if taps is not None:
            taps['layer%d' % (li + 1)] = _to_nchw(cur, n, H, W)
    return cur, H, W


def gce_eval(plan, x4, b, t, dp, taps=None):
    """x4 [b*t*128][2048] -> (x_uncorr, x_corr) same shape and storage, corr_map [b*t*128] (fp32, as every per-clip
    vector)."""
    M = x4.shape[0]
    _stage('gce')
    x_glo = _new((b, 2048), x4)
    _call(_k('grl_group_mean', x4), ptr(x4), ptr(x_glo), b, t * PIX, 2048, 2048, C.c_float(1.0), 0)
    # (the per-clip linears: fp32 operands on every datapath -- gemm()'s default math is MATH_F32 on bf16 storage)
    g = plan.glo_fc
    glo = _new((b, 1024), x4)
    gemm(x_glo, g.w, glo, b, 1024, 2048, scale=g.scale, shift=g.shift, relu=True, kblock=_kb())
    # W.[x; g] = Wx.x + Wg.g : the broadcast-concat of basebranch.py:59-61 becomes a
    # per-clip bias added inside the accumulator epilogue.
    c0 = plan.corr0
    gb = _new((b, 1024), x4)
    gemm(glo, c0.w[:, 2048:], gb, b, 1024, 1024, ldw=3072, kblock=_kb())
    h1 = _newl((M, 1024), x4)
    w0, m0 = _gw(c0, x4, dp, 2048)              # (the x4 half of corr0's [1024][3072] weight)
    gemm(x4, w0, h1, M, 1024, 2048, ldw=3072, gbias=gb, rows_per_group=t * PIX,
         scale=c0.scale, shift=c0.shift, relu=False, math=m0)
    c2 = plan.corr2
    h2 = _newl((M, 256), x4)
    w2, m2 = _gw(c2, x4, dp)
    gemm(h1, w2, h2, M, 256, 1024, scale=c2.scale, shift=c2.shift, relu=True, math=m2)
    cmap = _new((M,), x4)
    xc = _newl((M, 2048), x4)
    xu = _newl((M, 2048), x4)
    _call(_k('grl_gce_gate', x4), ptr(h2), ptr(plan.corr5_w), ptr(plan.corr6_scale), ptr(plan.corr6_shift),
          ptr(x4), ptr(cmap), ptr(xc), ptr(xu), M, 256, 2048)
    if taps is not None:
        taps['x_glo'], taps['glo'] = x_glo, glo
        taps['corr_map'] = cmap.view(b * t, 1, 16, 8)
    return xu, xc, cmap


# The two TRL directions (forward / backward in time, grl_model.py:170-208) are independent recurrences over
# their own weights: each step's GEMMs have M = B*128 rows -- 128..256 tiles, half a chip -- and six small
# latency-bound kernels.  They are issued on two HIP streams (fork after the shared inputs, join before the
# pooled outputs) so the chip runs one direction's GEMM next to the other's small kernels.  Same kernels,
# same per-direction order, per-direction scratch: bit-identical to the single-stream order
# (GRL_TRL_STREAMS=0, or taps requested).
TRL_STREAMS = os.environ.get('GRL_TRL_STREAMS', '1') != '0'
# Round 5 (eval): each direction's ATTENTION branch of a step -- the f1 GEMM with its squared-difference epilogue and the
# three latency-bound kernels behind it (partial-sum GAP, the two channel-attention layers) -- only reads the step's memo
# and feeds f_corr, never the recurrence; in stream order it still sat in front of the step's add / conv1 / conv2 / conv3.
# It goes to a stream of its own (one per direction), forked from the direction's stream where the memo is ready, so the
# recurrence's GEMMs run next to it (knock-out bound: the small kernels cost 0.27 ms of configs[2] although nothing waits
# for their results before the join; measured configs[2] 10.03 -> 9.93-9.97 ms).  bf16 storage only: the exact-fp32 step
# LOSES 1 % to it (14.47 -> 14.63 ms; with only the small kernels moved 14.60) -- its f1 GEMMs are four times longer and
# sharing CUs costs them more than the bubbles they fill.  Same kernels on the same operands: bit-identical.
# GRL_TRL_ATT_STREAMS=0: the attention branch stays on its direction's stream.
TRL_ATT_STREAMS = os.environ.get('GRL_TRL_ATT_STREAMS', '1') != '0'
_side_streams = {}
_att_streams = {}


class _TrlFork(object):
    """streams[di] for the two TRL directions; ``with fork.on(di):`` routes launches and allocations;
    ``with fork.att_on(di):`` routes to the direction's attention stream (ordered after everything issued so far on
    the direction's own stream)."""

    def __init__(self, dev, enable, att=False):
        self.main = torch.cuda.current_stream(dev)
        self.two = bool(enable and TRL_STREAMS)
        self.att = None
        self.held = []          # tensors an attention stream reads: kept alive until the join
        if self.two:
            key = (dev.index if dev.index is not None else torch.cuda.current_device())
            if key not in _side_streams:
                _side_streams[key] = torch.cuda.Stream(dev)
            self.side = _side_streams[key]
            if att and TRL_ATT_STREAMS:
                if key not in _att_streams:
                    _att_streams[key] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
                self.att = _att_streams[key]
        else:
            self.side = self.main

    def att_on(self, di, *reads):
        """``reads``: tensors of the direction's stream the branch reads (held until the join)."""
        if self.att is None:
            return self.on(di)
        ev = torch.cuda.Event()
        ev.record(self.side if di == 1 else self.main)
        self.att[di].wait_event(ev)
        self.held.extend(r for r in reads if r is not None)
        return torch.cuda.stream(self.att[di])

    def fork(self):
        if self.two:
            ev = torch.cuda.Event()
            ev.record(self.main)
            self.side.wait_event(ev)

    def on(self, di):
        return torch.cuda.stream(self.side if di == 1 else self.main)

    def join(self, *side_tensors):
        if self.two:
            for st in (self.side,) + (tuple(self.att) if self.att is not None else ()):
                ev = torch.cuda.Event()
                ev.record(st)
                self.main.wait_event(ev)
                if st is not self.side:
                    # blocks the attention streams read / write were allocated on the DIRECTION streams: once `held`
                    # is dropped the allocator may hand a side-stream block to the side stream's next launch, so the
                    # side stream is ordered behind the attention streams as well (main already is)
                    self.side.wait_event(ev)
            for x in side_tensors:
                x.record_stream(self.main)
            self.held = []


def trl_eval(plan, xu, xc, b, t, dp, taps=None):
    """xu, xc [b][t][128][2048] (flat, fp32 or bf16 storage) -> f_uncorr [b][2048], f_corr [b][t][2048] (fp32)."""
    Cc = 2048
    frame = PIX * Cc
    Mb = b * PIX
    b16 = xu.dtype == torch.bfloat16
    _stage('trl')
    memo0 = _newl((Mb, Cc), xu)
    _call(_k('grl_temporal_mean', xu), ptr(xu), ptr(memo0), b, t, frame)
    gapc = _new((b * t, Cc), xu)
    _call(_k('grl_group_mean', xc), ptr(xc), ptr(gapc), b * t, PIX, Cc, Cc, C.c_float(1.0), 0)
    # (attention streams on bf16 storage only: the exact-fp32 step loses 1 % to them, see TRL_ATT_STREAMS)
    fk = _TrlFork(xu.device, taps is None and len(plan.dirs) == 2, att=b16)
    fk.fork()
    # conv_f2(x_corr_i) does not depend on the recurrence: one GEMM over all T per direction
    f2, fc, scr = [], [], []
    for di, d in enumerate(plan.dirs):
        with fk.on(di):
            y = _newl((b * t * PIX, Cc), xu)
            wf2, mf2 = _gw(d['f2'], xu, dp)
            gemm(xc, wf2, y, b * t * PIX, Cc, Cc, shift=d['f2'].shift, relu=True, math=mf2)
            f2.append(y)
            # per-direction accumulators / scratch (a + b == b + a: summing the two directions' f_corr
            # contributions at the join gives the bits the shared accumulator got in either arrival order)
            # (two streams: each direction has its own accumulator and writes every (clip, frame) row exactly once -- no
            #  zero fill, the attention kernel stores instead of accumulating)
            fc.append(_new((b, t, Cc), xu) if fk.two else (torch.zeros((b, t, Cc), dtype=torch.float32, device=xu.device) if di == 0 else fc[0]))
            scr.append((_new((b, Cc), xu), _new((b, 128), xu)))
    memo = [memo0, memo0]
    catte = _new((b, Cc), xu) if taps is not None else None
    # d = GAP((ReLU(conv_f1(memo)) - f2_t)^2): the squared difference is reduced in the f1 GEMM's epilogue (32-row
    # partial sums), conv_f1's output never reaches HBM (grl_model.py:146-149).  On bf16 storage the 256 x 256 kernel
    # has that epilogue (round 3): it takes the step when Mb is a multiple of 256 on MATH_BF16S; MX-FP8 has none.
    sqdiff = FUSE_TRL_SQDIFF and (not b16 or (Mb % 256 == 0 and dp == MATH_BF16S))
    for i in range(t):
        for di, d in enumerate(plan.dirs):
            ti = i if di == 0 else t - 1 - i
            with fk.att_on(di, memo[di]):                       # the attention branch (its own stream where the fork has one)
                dvec, hid = scr[di]
                wf1, mf1 = _gw(d['f1'], xu, dp)
                if sqdiff:
                    dpart = _new((Mb // 32, Cc), xu)
                    gemm(memo[di], wf1, dpart, Mb, Cc, Cc, shift=d['f1'].shift, epilogue=EPI_SQDIFF,
                         res=f2[di][ti * PIX:], res_rows=PIX, res_gstride=t * PIX, math=mf1)
                    _call('grl_group_mean', ptr(dpart), ptr(dvec), b, PIX // 32, Cc, Cc, C.c_float(1.0 / 32.0), 0)      # (fp32 partial sums on either storage)
                else:
                    f1 = _newl((Mb, Cc), xu)
                    gemm(memo[di], wf1, f1, Mb, Cc, Cc, shift=d['f1'].shift, relu=True, math=mf1)
                    _call(_k('grl_sqdiff_mean', f1), ptr(f1), ptr(f2[di][ti * PIX:]), ptr(dvec), b, PIX, Cc, t * frame)
                _call('grl_channel_atte', ptr(dvec), ptr(d['w1']), ptr(d['w2t']), ptr(gapc[ti:]), t * Cc,
                      ptr(catte), ptr(fc[di].view(b * t, Cc)[ti:]), t * Cc, 0 if fk.two else 1, b, Cc, d['w1'].shape[0], ptr(hid))
                if taps is not None:
                    taps.setdefault(('fwd', 'bwd')[di] + '_catte', []).append(catte.clone())
            with fk.on(di):                                     # the recurrence
                s = _newl((Mb, Cc), xu)
                _call(_k('grl_add_strided', xu), ptr(memo[di]), ptr(xu.view(-1)[ti * frame:]), ptr(s), b, frame, t * frame)
                c1, c2, c3 = d['c1'], d['c2'], d['c3']
                (w1, m1), (w2, m2), (w3, m3) = _gw(c1, xu, dp), _gw(c2, xu, dp), _gw(c3, xu, dp)
                o = _newl((Mb, 512), xu)
                gemm(s, w1, o, Mb, 512, Cc, scale=c1.scale, shift=c1.shift, relu=True, math=m1)
                o2 = _newl((Mb, 512), xu)
                gemm(o, w2, o2, Mb, 512, 512, scale=c2.scale, shift=c2.shift, relu=True, math=m2)
                nm = _newl((Mb, Cc), xu)
                gemm(o2, w3, nm, Mb, Cc, 512, scale=c3.scale, shift=c3.shift, res=s, relu=True, math=m3)
                memo[di] = nm
    fk.join(memo[1], fc[1])
    fcorr = fc[0]
    if fk.two:
        fcorr = _new((b, t, Cc), xu)
        _call('grl_add_strided', ptr(fc[0]), ptr(fc[1]), ptr(fcorr), 1, b * t * Cc, 0)
    f_uncorr = _new((b, Cc), xu)
    _call(_k('grl_group_mean', memo[0]), ptr(memo[0]), ptr(f_uncorr), b, PIX, Cc, Cc, C.c_float(1.0), 0)
    _call(_k('grl_group_mean', memo[1]), ptr(memo[1]), ptr(f_uncorr), b, PIX, Cc, Cc, C.c_float(1.0), 1)
    if taps is not None:
        taps['f_uncorr'], taps['f_corr'] = f_uncorr, fcorr
    return f_uncorr, fcorr


def _grl_eval(model, inputs, taps=None, out_uncorr=None, ld_uncorr=2048):
    """The eval forward on the current datapath: MATH_BF16S / MATH_MXFP8 keep the activations bf16 in HBM from the stem
    to the TRL memo (and, MX-FP8, run the generic conv / linear GEMMs on MX operands: _gw); per-clip vectors and the
    BN1d + L2 tail are fp32 on every datapath."""
    dp = _math[0]
    plan = _plan(model, GrlEvalPlan)
    b, t, c, h, w = inputs.shape
    if (c, h, w) != (3, 256, 128):
        raise ValueError('GRL expects clips of [B,T,3,256,128] (got %s)' % (tuple(inputs.shape),))
    x = inputs.contiguous().view(b * t, c, h, w)
    x4, _, _ = trunk_eval(plan, x, dp, taps)
    xu, xc, _ = gce_eval(plan, x4, b, t, dp, taps)
    del x4
    f_uncorr, f_corr = trl_eval(plan, xu, xc, b, t, dp, taps)
    _stage('tail')
    x_corr = _new((b, t, 2048), inputs)
    _call('grl_affine_l2norm', ptr(f_corr), ptr(plan.corr_bn[0]), ptr(plan.corr_bn[1]), ptr(x_corr),
          b * t, 2048, 2048)
    x_uncorr = out_uncorr if out_uncorr is not None else _new((b, 2048), inputs)
    _call('grl_affine_l2norm', ptr(f_uncorr), ptr(plan.uncorr_bn[0]), ptr(plan.uncorr_bn[1]),
          ptr(x_uncorr), b, 2048, ld_uncorr)
    return x_uncorr, x_corr


def grl_forward(model, inputs, taps=None):
    """ResNet50_GRL_Model.forward.  eval(): folded-BN inference path.
    train(): batch-statistics forward recorded for the HIP backward."""
    require_device(inputs, 'inputs', allow_u8=True)
    if inputs.dim() != 5:
        raise ValueError('inputs must be [B,T,3,256,128]')
    if inputs.dtype == torch.uint8:
        inputs = rect_scale_u8(inputs)           # raw frames of another size: RectScale(256, 128) first
    if model.training:
        from . import train_engine
        return train_engine.grl_forward_train(model, normalize_u8(inputs))
    with torch.no_grad():
        return _grl_eval(model, inputs, taps)


# ----------------------------------------------------------------------------
# Siamese heads
# ----------------------------------------------------------------------------
def _attn_into(siam, x, out, ldy):
    plan = _plan(siam, SiameseEvalPlan)
    b, t, c = x.shape
    x = x.contiguous()
    qk = _new((b * t, 2 * plan.D), x)
    gemm(x, plan.wqk, qk, b * t, 2 * plan.D, c, scale=plan.scale, shift=plan.shift, kblock=_kb())
    _call('grl_siamese_attn', ptr(qk), ptr(x), ptr(out), b, t, plan.D, c, ldy)
    return out


def siamese_self_attention(siam, x):
    require_device(x, 'input')
    if siam.training:
        from . import train_engine
        return train_engine.siamese_self_attention_train(siam, x)
    with torch.no_grad():
        return _attn_into(siam, x, _new((x.shape[0], x.shape[2]), x), x.shape[2])


def siamese_forward(siam, x):
    require_device(x, 'input')
    from . import train_engine
    return train_engine.siamese_forward(siam, x)


def siamese_video_forward(siamv, x):
    require_device(x, 'input')
    from . import train_engine
    return train_engine.siamese_video_forward(siamv, x)


def extract_features(cnn, siam, clips):
    """attevaluator.py:100-112 in one pass: [b,T,3,256,128] -> [b,6144] =
    cat(x_uncorr, self_attention(x_corr), mean_T(x_corr)), each written straight
    into its slice of the feature row."""
    require_device(clips, 'clips', allow_u8=True)
    cnn = getattr(cnn, 'module', cnn)            # nn.DataParallel wrapper (mars_train.py:80)
    if cnn.training or siam.training:
        raise RuntimeError('extract_features needs cnn.eval() and siamese.eval()')
    with torch.no_grad():
        if clips.dtype == torch.uint8:
            clips = rect_scale_u8(clips)
        b, t = clips.shape[:2]
        feat = _new((b, 6144), clips)
        _, x_corr = _grl_eval(cnn, clips, out_uncorr=feat, ld_uncorr=6144)
        _attn_into(siam, x_corr, feat[:, 2048:], 6144)
        _call('grl_mean_T', ptr(x_corr), ptr(feat[:, 4096:]), b, t, 2048, 6144)
        return feat


def rows_mean(x):
    """[n, C] -> [1, C]: mean over rows (dense-mode clip average, attevaluator.py:96) through
    grl_group_mean."""
    require_device(x, 'features')
    x = x.contiguous()
    n, c = x.shape
    y = _new((1, c), x)
    _call('grl_group_mean', ptr(x), ptr(y), 1, n, c, c, C.c_float(1.0), 0)
    return y


class DevicePrefetcher(object):
    """Iterates a loader of (imgs, pids, camids) with the NEXT batch's host->device copy in flight
    on a side HIP stream while the current batch computes (pinned staging, non-blocking copy, an
    event hands the buffer to the compute stream).  uint8 batches stay uint8 (the stem normalises
    them, a quarter of the PCIe bytes); anything else is made float32 on the host, as
    `imgs.to(device)` upstream (attevaluator.py:70,76)."""

    def __init__(self, loader, device, depth=None, jpeg_size=(256, 128)):
        """``depth``: batches prepared ahead, each on its own side stream (default 1; 2 for loaders that hand over
        compressed frames).  ``jpeg_size``: the RectScale target (dataloader.py:53,68) that a compressed batch of MIXED
        frame sizes is brought to while it is decoded (jpeg.decode_jpeg_batch ``size``)."""
        import collections
        self.jpeg_size = jpeg_size
        self._ring = None
        self.it = iter(loader)
        self.dev = torch.device(device)
        self.depth = depth
        self.streams = []
        self._compressed = False
        self.queue = collections.deque()
        self._k = 0
        self._fill()

    def _stream(self):
        want = self.depth or 1
        while len(self.streams) < want:
            # NORMAL priority (GRL_PREFETCH_PRIORITY=-1: high, for A/B).  History: streams of one priority level share
            # GPU_MAX_HW_QUEUES (4) in-order hardware queues, and the first decoder's 10 ms entropy kernel on a normal-priority
            # prefetch stream sat in front of compute kernels of the SAME hardware queue (24.8 ms per eval step = 14.5 + 10.3);
            # high-priority streams have hardware queues of their own, which fixed that.  With the 0.8 ms decoder the
            # interference is gone -- and high priority has a cliff: a stream gets its hardware queue at FIRST USE, and when the
            # high-priority prefetch streams are used before the engine's side streams (a loader built before the first step:
            # the normal order), the normal-priority streams used afterwards serialise: bf16-storage train step 17.8 -> 32 ms,
            # fp32 53 -> 68, configs[2] eval 9.8 -> 12.2 (tools/jpeg_feed_order.py, profiles/r06_jpeg_feed_order.txt).
            pr = int(os.environ.get('GRL_PREFETCH_PRIORITY', '0')) if self._compressed else 0
            self.streams.append(torch.cuda.Stream(self.dev, priority=pr))
        self._k += 1
        return self.streams[self._k % want]

    def _fill(self):
        while len(self.queue) < (self.depth or 1):
            if not self._load():
                break

    def _load(self):
        try:
            imgs, pids, cams, *extra = next(self.it)   # extra: e.g. the augmentation parameter block
        except StopIteration:
            return False
        from grl_amd.reid.data.jpeg import JpegBatch, decode_jpeg_batch
        if isinstance(imgs, JpegBatch):
            # compressed frames (a loader with decode='device'): the bytes cross PCIe, grl_jpeg_decode_batch turns them
            # into the uint8 clip tensor on a prefetch stream, next to the current batch's compute (video_loader.py:124-141)
            if self.depth is None:
                self.depth = 2
            if not self._compressed:
                self._compressed, self.streams = True, []
            with torch.cuda.stream(self._stream()) as _:
                d = decode_jpeg_batch(imgs, self.dev, size=self.jpeg_size)
                ev = torch.cuda.Event()
                ev.record()
            self.queue.append((d, pids, cams, ev, None, extra))
            return True
        if imgs.dtype not in (torch.uint8, torch.float32):
            imgs = imgs.float()
        if imgs.is_cuda:
            self.queue.append((imgs, pids, cams, None, None, extra))
            return True
        host = imgs.contiguous()
        st = self._stream()
        with torch.cuda.stream(st):
            if host.is_pinned():                         # a loader with pin_memory=True (the reference's: dataloader.py:37-79)
                d = host.to(self.dev, non_blocking=True)
            else:
                # pageable batch: staged through a ring of reusable pinned buffers (no pinned allocation per batch) by ONE
                # host thread (below).  With `host.pin_memory()` here the bf16-storage training loop ran at 34.7 ms per
                # iteration on unpinned uint8 batches against 19.4 on pinned ones (tools/loop_rate.py)
                from grl_amd.reid.data.jpeg import _PinnedRing
                if self._ring is None:
                    self._ring = _PinnedRing()
                nbytes = host.numel() * host.element_size()
                slot, buf = self._ring.get(nbytes)
                stage = buf[:nbytes].view(host.dtype).view(host.shape)
                # ONE thread copies: `stage.copy_(host)` fans out over every OpenMP thread torch has (128 on the test boxes),
                # whose spin-waiting afterwards takes the cores from the thread that issues the step's ~1500 launches
                # (34.8 ms per bf16-storage iteration with copy_, the copy itself being 0.03 ms)
                C.memmove(stage.data_ptr(), host.data_ptr(), nbytes)
                d = stage.to(self.dev, non_blocking=True)
                self._ring.mark(slot)
                host = None
        ev = torch.cuda.Event()
        ev.record(st)
        self.queue.append((d, pids, cams, ev, host, extra))  # `host` kept alive until the copy is consumed
        return True

    def __iter__(self):
        return self

    def __next__(self):
        if not self.queue:
            raise StopIteration
        d, pids, cams, ev, _host, extra = self.queue.popleft()
        if ev is not None:
            cur = torch.cuda.current_stream(self.dev)
            cur.wait_event(ev)
            d.record_stream(cur)
        self._fill()
        return (d, pids, cams) + tuple(extra)


class GraphedExtractor(object):
    """`extract_features` captured once per input shape into a HIP graph (through
    torch.cuda.CUDAGraph: our launches go to torch's capturing stream) and replayed.
    One step is ~150 short launches; at small batches (the dense test_all.py mode feeds
    chunks of <= 8 clips, attevaluator.py:72-76) the host launch cost, not the GPU, bounds
    the eager path.  Output is bit-identical to the eager call (same kernels, same order).
    The packed-weight plans are built eagerly before capture and re-checked on every call:
    a parameter change drops the captured graphs."""

    def __init__(self, cnn, siam):
        self.cnn = getattr(cnn, 'module', cnn)
        self.siam = siam
        self._graphs = {}
        self._key = None

    def __call__(self, clips):
        require_device(clips, 'clips', allow_u8=True)
        key = (_state_key(self.cnn), _state_key(self.siam))
        if key != self._key:
            self._graphs.clear()
            self._key = key
        shape = tuple(clips.shape)
        g = self._graphs.get(shape)
        if g is None:
            static_in = clips.clone()
            for _ in range(2):                              # builds plans, warms the allocator
                extract_features(self.cnn, self.siam, static_in)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = extract_features(self.cnn, self.siam, static_in)
            g = (graph, static_in, static_out)
            self._graphs[shape] = g
        graph, static_in, static_out = g
        static_in.copy_(clips)
        graph.replay()
        return static_out.clone()


# ----------------------------------------------------------------------------
# evaluator distance matrices
# ----------------------------------------------------------------------------
def cosin_dist(qf, gf):
    """-qf . gf^T  (attevaluator.py:44-46) as one fp32 MFMA GEMM."""
    require_device(qf, 'qf'); require_device(gf, 'gf')
    qf, gf = qf.contiguous(), gf.contiguous()
    m, k = qf.shape
    n = gf.shape[0]
    out = _new((m, n), qf)
    return gemm(qf, gf, out, m, n, k, epilogue=EPI_NEGDOT, math=MATH_F32)


def pairwise_distance_tensor(x, y):
    """sqrt(clamp(|x|^2 + |y|^2 - 2 x.y^T, 1e-12))  (attevaluator.py:33-41)."""
    require_device(x, 'x'); require_device(y, 'y')
    m, n = x.shape[0], y.shape[0]
    x, y = x.contiguous().view(m, -1), y.contiguous().view(n, -1)
    k = x.shape[1]
    rn, cn = _new((m,), x), _new((n,), x)
    _call('grl_row_sqnorm', ptr(x), ptr(rn), m, k, k)
    _call('grl_row_sqnorm', ptr(y), ptr(cn), n, k, k)
    out = _new((m, n), x)
    return gemm(x, y, out, m, n, k, epilogue=EPI_EUCLID, rnorm=rn, cnorm=cn, math=MATH_F32)


def rank_rows(distmat):
    """Row-wise ascending argsort on the GPU (int32 [rows][n]); ties to the smaller index.
    Replaces the host `np.argsort(distmat, axis=1)` of eva_functions.py:139: one LDS bitonic
    network per row up to 16384 columns (MARS: 11310), the chunked network beyond (galleries of
    up to 2^24 entries; rows are processed in slabs so the workspace stays below ~1 GB)."""
    require_device(distmat, 'distmat')
    distmat = distmat.contiguous()
    rows, n = distmat.shape
    idx = torch.empty((rows, n), dtype=torch.int32, device=distmat.device)
    if n <= 16384:
        _call('grl_row_argsort', ptr(distmat), n, rows, n, ptr(idx))
        return idx
    lib = _lib.load()
    per_row = lib.grl_row_argsort_workspace_bytes(1, n)
    slab = max(1, min(rows, 65535, (1 << 30) // per_row))
    ws = torch.empty(lib.grl_row_argsort_workspace_bytes(slab, n), dtype=torch.uint8, device=distmat.device)
    for r0 in range(0, rows, slab):
        r = min(slab, rows - r0)
        _call('grl_row_argsort_wide', ptr(distmat[r0:]), n, r, n, ptr(idx[r0:]), ptr(ws))
    return idx


def rank_metrics(indices, q_pids, g_pids, q_camids, g_camids, max_rank=100):
    """CMC curve and mAP of eva_functions.evaluate (eva_functions.py:134-184) from a device
    argsort (``rank_rows``): `grl_rank_metrics` leaves (first match rank, #matches, AP) per query,
    the host only averages nq numbers.  Returns (cmc[max_rank] float32, mAP float)."""
    import numpy as np
    if not (torch.is_tensor(indices) and indices.is_cuda and indices.dtype == torch.int32):
        raise _lib.GrlHipError('rank_metrics needs the int32 device index matrix of rank_rows')
    indices = indices.contiguous()
    nq, ng = indices.shape
    dev = indices.device

    qp, qc = _ids(q_pids, nq, 'q_pids', dev), _ids(q_camids, nq, 'q_camids', dev)
    gp, gc = _ids(g_pids, ng, 'g_pids', dev), _ids(g_camids, ng, 'g_camids', dev)
    first = torch.empty(nq, dtype=torch.int32, device=dev)
    nhit = torch.empty(nq, dtype=torch.int32, device=dev)
    ap = torch.empty(nq, dtype=torch.float64, device=dev)
    _call('grl_rank_metrics', ptr(indices), ng, ptr(qp), ptr(qc), ptr(gp), ptr(gc), nq, ng, ptr(first), ptr(nhit),
          ptr(ap))
    return _cmc_map(first, nhit, ap, ng, max_rank)


def _ids(a, n, what, dev=None):
    """A pid / camera id list as int32 [n]: a numpy array, or a tensor on ``dev``.  The kernels compare ids as
    int32, so a value outside that range is refused rather than wrapped."""
    import numpy as np
    a = np.asarray(a).reshape(-1)
    if a.size != n:
        raise ValueError('%s: expected %d entries, got %d' % (what, n, a.size))
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError('%s: ids must fit int32' % what)
    a = a.astype(np.int32)
    return a if dev is None else torch.from_numpy(a).to(dev)


def _cmc_map(first, nhit, ap, ng, max_rank):
    """(cmc[max_rank] float32, mAP) from the per-query (first match rank, #matches, AP) device arrays."""
    import numpy as np
    first, nhit, ap = first.cpu().numpy(), nhit.cpu().numpy(), ap.cpu().numpy()
    valid = nhit > 0
    assert valid.any(), "Error: all query identities do not appear in gallery"
    if ng < max_rank:
        max_rank = ng
        print("Note: number of gallery samples is quite small, got {}".format(ng))
    hit_by = (first[valid][:, None] <= np.arange(max_rank)[None, :]).astype(np.float32)
    return hit_by.sum(0) / float(valid.sum()), float(np.mean(ap[valid]))



# ----------------------------------------------------------------------------
# ranking by the Siamese verification head (verify.hip)
# ----------------------------------------------------------------------------
class VerifyFoldPlan(EvalPlan):
    """classifierBN -> classifierlinear of a Siamese in eval mode, folded to the weights ``w`` [D] (fp32) and the
    constant ``c`` (fp64 and fp32 copies, on the device) of the logit difference s(p, g) = sum_d w_d (p_d - g_d)^2 + c
    (grl_verify_fold).  Cached by ``_plan``: rebuilt when a parameter or a running statistic of the module changes."""

    def __init__(self, siam):
        super().__init__(siam)
        bn, lin = siam.classifierBN, siam.classifierlinear
        self.D = D = bn.num_features
        self.w = torch.empty(D, dtype=torch.float32, device=self.dev)
        self.c64 = torch.empty(1, dtype=torch.float64, device=self.dev)
        self.c32 = torch.empty(1, dtype=torch.float32, device=self.dev)
        W, b = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()
        _call('grl_verify_fold', ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
              C.byref(C.c_double(bn.eps)), ptr(W), ptr(b), D, ptr(self.w), ptr(self.c64), ptr(self.c32))


class VerifyMetric(object):
    """The ranking distance F(q, g) = (1 - beta) (-q . g) - beta s(p, g) of ``verify_metric``: what ``_ColumnBlocks``,
    ``search``, ``rank_metrics_streaming`` and ``verify_dist`` take as ``metric``.  It holds the module, not the folded
    numbers: ``folded()`` goes through the plan cache, so a weight update is picked up by the next call."""

    def __init__(self, siam, col0, beta):
        self.siam, self.col0, self.beta = siam, col0, beta
        self.Dv = siam.classifierBN.num_features

    def folded(self):
        """(w [Dv] fp32, c fp64 [1], c fp32 [1]) on the device."""
        p = _plan(self.siam, VerifyFoldPlan)
        return p.w, p.c64, p.c32

    @property
    def full(self):
        """beta < 1: the GEMM runs over the whole row; beta == 1: over the head's slice only."""
        return self.beta < 1.0

    def check_rows(self, d):
        """ValueError unless rows of ``d`` columns hold the slice and the NEGDOT GEMM takes the resulting K."""
        if self.col0 + self.Dv > d:
            raise ValueError('verify metric: the slice [%d, %d) does not fit rows of %d columns'
                             % (self.col0, self.col0 + self.Dv, d))
        if d % 4 or (self.full and d % 32):
            raise ValueError('verify metric: feature rows of %d columns (the distance GEMM needs a multiple of %d)'
                             % (d, 32 if self.full else 4))

    def __repr__(self):
        return 'verify(col0=%d, Dv=%d, beta=%r)' % (self.col0, self.Dv, self.beta)


def verify_metric(siam, col0, beta=1.0):
    """Rank by the trained pair-verification head of ``siam`` (classifierBN + classifierlinear, eval mode) instead of
    the cosine distance.  With p, g = columns [col0, col0 + input_num) of a query / gallery row, the head's class-1
    minus class-0 logit is s(p, g) = sum_d w_d (p_d - g_d)^2 + c and sigmoid(s) is the trainer's pair probability; the
    returned metric is F(q, g) = (1 - beta) (-q . g) + beta (-s(p, g)), 0 < beta <= 1 (beta = 1: the head alone).  It is
    accepted as ``metric`` by ``search``, ``rank_metrics_streaming`` (and their sharded forms) and ``verify_dist``; the
    pairs x d tensor of (p - g)^2 is never built.  ValueError: a head with class_num != 2, beta outside
    (0, 1], a negative or unaligned col0, a head width the kernels or the GEMM cannot take."""
    ncls = siam.classifierlinear.out_features
    if ncls != 2:
        raise ValueError('verify_metric: the head has class_num = %d; the logit difference needs 2' % ncls)
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0.0 < float(beta) <= 1.0:
        raise ValueError('verify_metric: beta must be a number in (0, 1] (got %r)' % (beta,))
    if isinstance(col0, bool) or not isinstance(col0, numbers.Integral) or col0 < 0 or col0 % 4:
        raise ValueError('verify_metric: col0 must be a non-negative multiple of 4 (got %r)' % (col0,))
    Dv = siam.classifierBN.num_features
    if siam.classifierlinear.in_features != Dv:
        raise ValueError('verify_metric: classifierBN has %d features, classifierlinear takes %d'
                         % (Dv, siam.classifierlinear.in_features))
    if Dv % 32:           # beta = 1 runs the GEMM over K = Dv; the row kernel reads 16 bytes at a time
        raise ValueError('verify_metric: a head of width %d (the distance GEMM needs K %% 32 == 0)' % Dv)
    if siam.training:
        raise RuntimeError('verify_metric needs siamese.eval(): the fold uses the running statistics')
    return VerifyMetric(siam, int(col0), float(beta))


def verify_dist(qf, gf, metric):
    """The materialised [nq, ng] matrix of ``metric`` (a ``verify_metric``): one column block of ``_ColumnBlocks``,
    so every entry has the bits ``search`` and ``rank_metrics_streaming`` see.  Not collective: under
    torch.distributed shard the gallery rows with grl_amd.dist.sharded_distmat, as for cosin_dist."""
    if not isinstance(metric, VerifyMetric):
        raise ValueError('verify_dist: metric must come from verify_metric (got %r)' % (metric,))
    nq, ng = qf.shape[0], gf.shape[0]
    blocks = _ColumnBlocks(qf, gf, metric, block_cols=max(ng, 1))
    if nq == 0 or ng == 0:
        return _new((nq, ng), blocks.qf)
    return blocks.block(0, ng)


def verify_prob(dist):
    """sigmoid(-dist): the head's probability that a pair shows the same person, for the distances of a pure-head
    metric (beta = 1; a blend has no such reading) -- a matrix of ``verify_dist`` or the lists of ``search``.  A
    convenience for thresholding; padding (+inf) becomes 0."""
    if torch.is_tensor(dist):
        return torch.sigmoid(-dist)
    import numpy as np
    d = np.asarray(dist, dtype=np.float64)
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(d))


# ----------------------------------------------------------------------------
# gallery search and ranking metrics over column blocks (search.hip)
# ----------------------------------------------------------------------------
SEARCH_BLOCK_BYTES = int(os.environ.get('GRL_SEARCH_BLOCK_BYTES', str(256 << 20)))   # distance block budget
SEARCH_K_MAX = 1024
_INT_MAX = 2 ** 31 - 1               # what a C int of the ABI holds


def _int_arg(v, lo, hi, what, name, bound=None):
    """``v`` as an int, or ValueError: an integer (never a bool) in lo..hi; ``hi`` None = no upper limit.  The message
    names the range as 'in lo..hi', as '>= lo' without ``hi``, or as ``bound`` where the caller words it."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or (hi is not None and v > hi):
        if bound is None:
            bound = '>= %d' % lo if hi is None else 'in %d..%d' % (lo, hi)
        raise ValueError('%s: %s must be an integer %s (got %r)' % (what, name, bound, v))
    return int(v)


def _search_k(k, what):
    """The list length ``k`` of a search as an int, or ValueError: 1 <= k <= SEARCH_K_MAX, not a bool."""
    if isinstance(k, bool) or not 1 <= int(k) <= SEARCH_K_MAX:
        raise ValueError('%s: k must be in 1..%d (got %r)' % (what, SEARCH_K_MAX, k))
    return int(k)


def _check_index(index, cls, what):
    if not isinstance(index, cls):
        name = cls.__name__
        raise ValueError('%s: index must be %s %s (got %s)' % (what, 'an' if name[0] in 'AEIOU' else 'a', name,
                                                               type(index).__name__))


def _block_budget(block_bytes):
    """The bytes one distance block may take: ``block_bytes``, or GRL_SEARCH_BLOCK_BYTES as it stands at the call."""
    return SEARCH_BLOCK_BYTES if block_bytes is None else int(block_bytes)


def _block_cols(nq, block_bytes, granule=256):
    """The default block width: the float32 columns of ``nq`` rows that fit the budget, rounded down to a multiple of
    ``granule`` and at least one granule; ``granule`` None: as many as fit, unrounded (0 when not even one does)."""
    cols = _block_budget(block_bytes) // (4 * max(nq, 1))
    return max(granule, cols // granule * granule) if granule else cols


def _block_spans(nq, lo, hi, block_cols=None, block_bytes=None, granule=256):
    """``(width, spans)``: the columns [lo, hi) cut into blocks of ``block_cols`` (default ``_block_cols``) columns, the
    last one shorter; the width is at least 1 and at most hi - lo."""
    if block_cols is None:
        block_cols = _block_cols(nq, block_bytes, granule)
    width = max(1, min(int(block_cols), hi - lo))
    return width, [(c, min(c + width, hi)) for c in range(lo, hi, width)]


def _sample_block_cols(n, block_bytes):
    """The default width of the n x n sample passes (``_SampleBlocks``, ``_JaccardSet``): the multiple of 32 samples whose
    three buffers fit the budget, and never the whole matrix in one block."""
    cols = max(32, _block_budget(block_bytes) // (12 * n) // 32 * 32)
    return min(cols, max(32, -(-n // 64) * 32))


class _BlockSource(object):
    """The block-source contract, which every streamed consumer (``_search_blocks``, ``_rank_blocks``,
    ``_roc_blocks``, ``_eps_graph_blocks``, ``_mst_blocks``, ``_dist_from_blocks``) relies on.  A source provides

      qf, nq         the query rows (a device tensor: consumers take the device from it) and their number
      spans          [(c0, c1), ...]: the source's columns in ascending, disjoint blocks
      block(c0, c1)  the [nq, c1 - c0] float32 distances of one span, a view of the ONE reused buffer ``buf``: valid
                     until the next ``block`` call, and the consumer may overwrite it

    A block comes back with the same bits every time it is asked for (the two-pass consumers ask twice), and an entry's
    bits do not depend on the block width: every width gives the full matrix's bits.  ``_cut`` is the one width rule:
    ``block_cols`` columns, else what fits ``block_bytes`` (``_block_cols``)."""

    def _cut(self, lo, hi, block_cols, block_bytes, granule=256):
        """``width``, ``spans`` and ``buf`` for the columns [lo, hi); ``nq`` and ``qf`` are set already."""
        self.width, self.spans = _block_spans(self.nq, lo, hi, block_cols, block_bytes, granule)
        self.buf = _new((self.nq * self.width,), self.qf) if self.spans and self.nq else None

    def _view(self, n):
        """the [nq, n] view of the buffer that a block of ``n`` columns is written to"""
        return self.buf[:self.nq * n].view(self.nq, n)


class _TopK(object):
    """The running top-k lists of ``n`` rows as grl_topk_block keeps them: ``key`` int64 [n, k], the composites (all ones
    = an empty slot), and ``val`` float32 [n, k] (+inf there)."""

    def __init__(self, n, k, dev):
        self.n, self.k = n, k
        self.key = torch.full((n, k), -1, dtype=torch.int64, device=dev)
        self.val = torch.full((n, k), float('inf'), dtype=torch.float32, device=dev)

    def push(self, d, ld, ncols, c0, cidx=None, ldc=0, junk=None, rows=None):
        """Merge the block ``d`` (``ncols`` columns, row stride ``ld``; column j is entry ``c0 + j``, or ``cidx[.][j]``
        with ``cidx`` int32 of row stride ``ldc``, < 0 = skipped) into the lists of all rows, or of ``rows = (q0, q1)``.
        ``junk``: the arrays of ``_junk_ids`` for all n rows; the block then goes through grl_topk_block_filtered."""
        key, val, nrows = self.key, self.val, self.n
        if rows is not None:
            q0, nrows = rows[0], rows[1] - rows[0]
            key, val = key[q0:], val[q0:]
            if junk is not None:
                junk = (junk[0][q0:], junk[1][q0:], junk[2], junk[3])
        args = (ptr(d), ld, ptr(cidx), ldc, nrows, ncols, c0, self.k, ptr(key), ptr(val))
        if junk is None:
            _call('grl_topk_block', *args)
        else:
            _call('grl_topk_block_filtered', *args + (ptr(junk[0]), ptr(junk[1]), ptr(junk[2]), ptr(junk[3])))

    def result(self):
        """``(dist [n, k] float32, idx [n, k] int64)`` as ``search`` returns them: an empty slot is index -1, +inf."""
        idx = self.key & 0xffffffff
        idx[idx == 0xffffffff] = -1
        return self.val, idx


class _ColumnBlocks(_BlockSource):
    """Column blocks D[:, c0:c1] of the distance matrix of ``qf`` against gallery rows [lo, hi) of ``gf``
    ('cosine' = cosin_dist, 'euclidean' = pairwise_distance_tensor), one GEMM per block into one reused
    buffer.  Every entry is computed by the same fma chain as in the full matrix (the GEMM's order does not
    depend on N; no split-K scratch is handed over), so a block holds the full matrix's bits.  Without
    ``block_cols`` the width is the largest multiple of 256 columns whose block fits ``block_bytes``.
    ``metric`` may also be a ``verify_metric``: the constructor prepares the modified queries q' and the row terms
    rq, rg (for the gallery rows [lo, hi) only), a block is the NEGDOT GEMM of q' and grl_verify_finish on it."""

    def __init__(self, qf, gf, metric='cosine', block_cols=None, block_bytes=None, lo=0, hi=None):
        vm = metric if isinstance(metric, VerifyMetric) else None
        if vm is None and metric not in ('cosine', 'euclidean'):
            raise ValueError("metric must be 'cosine', 'euclidean' or a verify_metric (got %r)" % (metric,))
        if vm is not None:
            vm.check_rows(int(torch.Size(qf.shape[1:]).numel()))
        require_device(qf, 'qf'); require_device(gf, 'gf')
        nq, ng = qf.shape[0], gf.shape[0]
        self.qf = qf.contiguous().view(nq, torch.Size(qf.shape[1:]).numel())      # (-1 cannot be inferred for 0 rows)
        self.gf = gf.contiguous().view(ng, torch.Size(gf.shape[1:]).numel())
        if self.qf.shape[1] != self.gf.shape[1]:
            raise ValueError('qf and gf have different feature sizes (%d, %d)' % (self.qf.shape[1], self.gf.shape[1]))
        hi = ng if hi is None else hi
        self.nq, self.ng, self.metric = nq, ng, metric
        self._cut(lo, hi, block_cols, block_bytes)
        self.rn = self.cn = None
        if metric == 'euclidean' and self.spans and nq:
            k = self.qf.shape[1]
            self.rn, self.cn = _new((nq,), self.qf), _new((hi - lo,), self.qf)
            _call('grl_row_sqnorm', ptr(self.qf), ptr(self.rn), nq, k, k)
            _call('grl_row_sqnorm', ptr(self.gf[lo:hi]), ptr(self.cn), hi - lo, k, k)
        self.lo = lo
        self.qv = self.rq = self.rg = None
        if vm is not None:
            d = self.qf.shape[1]
            if self.spans and nq:
                w, c64, _ = vm.folded()
                beta, full = C.byref(C.c_double(vm.beta)), vm.full     # (a host double, read during the call)
                self.qv = _new((nq, d if full else vm.Dv), self.qf)
                self.rq, self.rg = _new((nq,), self.qf), _new((hi - lo,), self.qf)
                _call('grl_verify_rows', ptr(self.qf), d, nq, d, vm.col0, vm.Dv, ptr(w), beta, ptr(c64), ptr(self.rq),
                      ptr(self.qv), self.qv.shape[1], 1 if full else 0)
                _call('grl_verify_rows', ptr(self.gf[lo:hi]), d, hi - lo, d, vm.col0, vm.Dv, ptr(w), beta, None,
                      ptr(self.rg), None, 0, 0)

    def block(self, c0, c1):
        n, k = c1 - c0, self.qf.shape[1]
        out = self._view(n)
        if self.qv is not None:
            vm = self.metric
            if vm.full:
                gemm(self.qv, self.gf[c0:c1], out, self.nq, n, k, epilogue=EPI_NEGDOT, math=MATH_F32)
            else:               # beta = 1: K = the head's width, the gallery slice read in place through ldw
                gemm(self.qv, self.gf[c0:c1, vm.col0:], out, self.nq, n, vm.Dv, ldw=k, epilogue=EPI_NEGDOT,
                     math=MATH_F32)
            _call('grl_verify_finish', ptr(out), n, self.nq, n, ptr(self.rq), ptr(self.rg), c0 - self.lo)
            return out
        if self.metric == 'cosine':
            return gemm(self.qf, self.gf[c0:c1], out, self.nq, n, k, epilogue=EPI_NEGDOT, math=MATH_F32)
        return gemm(self.qf, self.gf[c0:c1], out, self.nq, n, k, epilogue=EPI_EUCLID, rnorm=self.rn,
                    cnorm=self.cn[c0 - self.lo:c1 - self.lo], math=MATH_F32)


def _shard(ng):
    from . import dist as grl_dist
    if not grl_dist.is_distributed():
        return 0, ng, False
    import torch.distributed as tdist
    lo, hi = grl_dist.shard_rows(ng, tdist.get_rank(), tdist.get_world_size())
    return lo, hi, True


def _junk_ids(exclude, nq, ng, dev):
    """``exclude = (q_pids, g_pids, q_camids, g_camids)`` (rank_metrics' order) as the int32 device arrays
    (q_pids, q_cams, g_pids, g_cams) of grl_topk_block_filtered; None stays None."""
    if exclude is None:
        return None
    if len(exclude) != 4:
        raise ValueError('exclude must be (q_pids, g_pids, q_camids, g_camids)')
    q_pids, g_pids, q_camids, g_camids = exclude
    return (_ids(q_pids, nq, 'q_pids', dev), _ids(q_camids, nq, 'q_camids', dev), _ids(g_pids, ng, 'g_pids', dev),
            _ids(g_camids, ng, 'g_camids', dev))


def search(qf, gf, k, metric='cosine', exclude=None, block_cols=None, block_bytes=None):
    """Each query's ``k`` nearest gallery entries: ``(dist [nq, k] float32, idx [nq, k] int64)`` on the device,
    without the query x gallery matrix.  Exactly ``rank_rows(D)[:, :k]`` and ``D`` at those indices, bit for
    bit, for D = cosin_dist(qf, gf) ('cosine') or pairwise_distance_tensor(qf, gf) ('euclidean'): canonical
    NaN, -0 == +0, ties to the smaller gallery index.  With fewer than ``k`` gallery entries the tail of every
    row is padding: index -1, distance +inf.  k <= 1024.  The distances are computed in column blocks of
    ``block_cols`` (default: as many as fit ``block_bytes``, GRL_SEARCH_BLOCK_BYTES, 256 MiB).  Under
    torch.distributed the gallery rows are sharded over the ranks and only the per-rank top-k lists are
    exchanged.

    ``exclude = (q_pids, g_pids, q_camids, g_camids)`` (the order of ``rank_metrics``) drops, for every query, the
    gallery entries that share its pid AND its camera: the junk rule of eva_functions.evaluate, which CMC / mAP and
    visualize_ranked_results apply.  Row q is then ``rank_rows(D)[q]`` with the junk entries of query q deleted,
    truncated to ``k`` (padded as above when fewer are left), and ``D`` at those indices, bit for bit.  The rule is
    applied on the device while the blocks are ranked (grl_topk_block_filtered); no nq x ng mask is built.
    ``exclude=None`` makes the calls it made before the argument existed."""
    k = _search_k(k, 'search')
    nq, ng = qf.shape[0], gf.shape[0]
    junk = _junk_ids(exclude, nq, ng, qf.device)
    lo, hi, sharded = _shard(ng)
    blocks = _ColumnBlocks(qf, gf, metric, block_cols, block_bytes, lo, hi)
    return _search_blocks(blocks, nq, k, sharded, junk)


def _search_blocks(blocks, nq, k, sharded, junk=None):
    """The running top-k of search over a block source (``_BlockSource``).  ``junk``: the device arrays of _junk_ids;
    every distance block then goes through grl_topk_block_filtered.  The merge of the ranks' lists stays unfiltered: its
    inputs are clean already."""
    top = _TopK(nq, k, blocks.qf.device)
    if nq == 0:
        return top.result()
    for c0, c1 in blocks.spans:
        top.push(blocks.block(c0, c1), c1 - c0, c1 - c0, c0, junk=junk)
    if sharded:
        import torch.distributed as tdist
        from . import dist as grl_dist
        world = tdist.get_world_size()
        vals = [torch.empty_like(top.val) for _ in range(world)]
        keys = [torch.empty_like(top.key) for _ in range(world)]
        grl_dist._all_gather(vals, top.val)
        grl_dist._all_gather(keys, top.key)
        cand_v = torch.cat(vals, 1).contiguous()                         # rank order; the merge is order-free
        cand_i = (torch.cat(keys, 1) & 0xffffffff).to(torch.int32).contiguous()   # empty slots: -1 = skipped
        top.key.fill_(-1)
        top.val.fill_(float('inf'))
        top.push(cand_v, world * k, world * k, 0, cand_i, world * k)
    return top.result()


def _dist_from_blocks(blocks, n):
    """The materialised [nq, n] matrix of a block source over the columns [0, n)."""
    out = _new((blocks.nq, n), blocks.qf)
    if blocks.nq:
        for c0, c1 in blocks.spans:
            out[:, c0:c1] = blocks.block(c0, c1)
    return out


def _search_by_query_rows(make_blocks, qf, rows, k, junk):
    """``_search_blocks`` (unsharded) over ``make_blocks(qf[q0:q1])`` for chunks of ``rows`` query rows, whose results
    are independent and concatenated: for sources that keep per-query state (tables) within a byte limit."""
    nq = qf.shape[0]
    dist, idx = [], []
    for q0 in range(0, max(nq, 1), rows):
        q1 = min(q0 + rows, nq)
        blocks = make_blocks(qf[q0:q1])
        j = None if junk is None else (junk[0][q0:q1], junk[1][q0:q1], junk[2], junk[3])
        dv, di = _search_blocks(blocks, q1 - q0, k, False, j)
        dist.append(dv)
        idx.append(di)
    return (dist[0], idx[0]) if len(dist) == 1 else (torch.cat(dist), torch.cat(idx))


def _metrics_from_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, max_rank, sharded):
    """(cmc[max_rank] float32, mAP float) of the distances of a block source: the tail of every *_metrics_streaming."""
    first, nhit, ap = _rank_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, sharded)
    return _cmc_map(first, nhit, ap, ng, max_rank)


def _two_stage(what, qf, index, d, metric, store, k, R, shortlist, block_bytes):
    """The checks of a two-stage search that all indexes share (the store is a RefineStore of the index's rows, 1 <= k <=
    R <= 1024), then ``refine_lists`` on the index lists of ``shortlist(R)``, the first stage's (dist, idx)."""
    if not isinstance(store, RefineStore):
        raise ValueError('%s: store must be a RefineStore (got %s)' % (what, type(store).__name__))
    if store.n != index.n or store.d != d:
        raise ValueError('%s: store must hold the rows of the index: store is [%d, %d], the index [%d, %d]'
                         % (what, store.n, store.d, index.n, d))
    k = _int_arg(k, 1, SEARCH_K_MAX, what, 'k')
    R = _int_arg(R, k, SEARCH_K_MAX, what, 'R (k <= R <= %d)' % SEARCH_K_MAX)
    return refine_lists(qf, store, shortlist(R)[1], k, metric, block_bytes)


# ----------------------------------------------------------------------------
# query expansion and database-side augmentation (expand.hip)
# ----------------------------------------------------------------------------
EXPAND_ALPHA_MAX = 8


def _expand_args(m, alpha, m_max, what):
    """(m, alpha) as ints, or ValueError: 1 <= m <= m_max, 0 <= alpha <= 8, both integers."""
    for name, v in (('m', m), ('alpha', alpha)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError('%s: %s must be an integer (got %r)' % (what, name, v))
    if not 1 <= m <= m_max:
        raise ValueError('%s: m must be in 1..%d (got %r)' % (what, m_max, m))
    if not 0 <= alpha <= EXPAND_ALPHA_MAX:
        raise ValueError('%s: alpha must be in 0..%d (got %r)' % (what, EXPAND_ALPHA_MAX, alpha))
    return int(m), int(alpha)


def expand_from_lists(xf, bank, dist, idx, m, alpha=0, skip_self=False):
    """A new [n, d] float32 tensor: row i is the weighted mean of ``xf[i]`` (weight 1) and its first ``m`` kept
    neighbours ``bank[idx[i, t]]`` of the lists ``(dist, idx)`` [n, L] (``search``'s return values: float32 distances,
    int64 indices, -1 = padding; with ``skip_self`` the entry idx == i is skipped, which needs xf and bank to have the
    same rows).  Weight of a neighbour: 1 for ``alpha`` == 0, else max(-dist, 0) ** alpha by alpha - 1 products
    (for 'cosine' lists -dist is the dot product).  One grl_expand_rows launch: the n x m x d gather ``bank[idx]`` is
    never built, and the summation order is fixed (tests/expand_ref.py reproduces it bit for bit)."""
    if idx.dim() != 2 or tuple(dist.shape) != tuple(idx.shape) or idx.shape[0] != xf.shape[0]:
        raise ValueError('expand_from_lists: dist and idx must both be [%d, L] (got %s, %s)'
                         % (xf.shape[0], tuple(dist.shape), tuple(idx.shape)))
    m, alpha = _expand_args(m, alpha, idx.shape[1], 'expand_from_lists')
    if skip_self and xf.shape[0] != bank.shape[0]:
        raise ValueError('expand_from_lists: skip_self needs xf and bank to have the same rows (got %d, %d)'
                         % (xf.shape[0], bank.shape[0]))
    require_device(xf, 'xf'); require_device(bank, 'bank'); require_device(dist, 'dist')
    if not (idx.is_cuda and idx.dtype == torch.int64):
        raise _lib.GrlHipError('expand_from_lists needs the int64 device index lists of search')
    n, nb = xf.shape[0], bank.shape[0]
    xf, bank = xf.contiguous().view(n, -1), bank.contiguous().view(nb, -1)
    if xf.shape[1] != bank.shape[1]:
        raise ValueError('xf and bank have different feature sizes (%d, %d)' % (xf.shape[1], bank.shape[1]))
    d, L = xf.shape[1], idx.shape[1]
    out = _new((n, d), xf)
    if n == 0:
        return out
    dist, idx = dist.contiguous(), idx.contiguous()
    _call('grl_expand_rows', ptr(xf), d, ptr(bank), d, ptr(idx), ptr(dist), L, n, nb, d, L, m, alpha,
          1 if skip_self else 0, ptr(out), d)
    return out


def expand_features(xf, bank, m, alpha=0, metric='cosine', exclude=None, skip_self=False, block_cols=None,
                    block_bytes=None):
    """Query expansion (AQE, alpha-QE) / database-side augmentation of feature rows, on the device: ``search(xf, bank,
    m + (1 if skip_self else 0), metric, exclude, ...)`` and ``expand_from_lists`` on its lists.  Row i of the result is
    (xf[i] + sum_p w_p bank[j_p]) / (1 + sum_p w_p) over its ``m`` nearest bank rows j_p; w_p = 1 (``alpha`` = 0) or
    (xf[i] . bank[j_p]) ** alpha clamped at 0 (``alpha`` in 1..8, 'cosine' only: 'euclidean' lists carry no similarity
    and take alpha = 0).  1 <= m <= SEARCH_K_MAX - 1.  ``skip_self``: xf IS bank (DBA), row i does not expand with
    itself -- the search asks for one more neighbour and the kernel drops the entry idx == i.  ``exclude`` has
    ``search``'s meaning (the evaluator's junk rule: same pid AND camera).  The result is a new tensor; xf and bank are
    only read.  Under torch.distributed ``search`` is collective and returns identical lists on every rank; every rank
    then expands all rows itself, so the result is identical on every rank with no further exchange."""
    m, alpha = _expand_args(m, alpha, SEARCH_K_MAX - 1, 'expand_features')
    if metric not in ('cosine', 'euclidean'):
        raise ValueError("metric must be 'cosine' or 'euclidean' (got %r)" % (metric,))
    if alpha > 0 and metric != 'cosine':
        raise ValueError("expand_features: alpha > 0 weights by the cosine similarity and needs metric='cosine' "
                         "(got alpha = %d with %r)" % (alpha, metric))
    if skip_self and xf.shape[0] != bank.shape[0]:
        raise ValueError('expand_features: skip_self needs xf and bank to have the same rows (got %d, %d)'
                         % (xf.shape[0], bank.shape[0]))
    dist, idx = search(xf, bank, m + (1 if skip_self else 0), metric=metric, exclude=exclude, block_cols=block_cols,
                       block_bytes=block_bytes)
    return expand_from_lists(xf, bank, dist, idx, m, alpha, skip_self)


def rank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, metric='cosine', max_rank=100,
                           block_cols=None, block_bytes=None):
    """``rank_metrics(rank_rows(D), ...)`` without D or its argsort: (cmc[max_rank] float32, mAP float) of
    eva_functions.evaluate for D = cosin_dist(qf, gf) / pairwise_distance_tensor(qf, gf).  Per query, the
    distances of its matches (its pid, another camera; same pid and camera is dropped) are gathered and sorted
    in a first pass over the column blocks; a second pass counts, for each non-match, how many matches come
    before it, and the matches' ranks follow from a prefix sum.  First-match rank and #matches per query are
    those of rank_metrics exactly, AP agrees to ~1e-15 (fp64, another summation order), so the CMC is equal and
    the mAP within 1e-12.  One GEMM pass when the whole matrix fits one block, two otherwise.  At most 8192
    gallery entries may share a query's pid.  Under torch.distributed the gallery rows are sharded over the
    ranks; they exchange only the match keys and the rank histograms (both sized by the matches)."""
    first, nhit, ap = _rank_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, metric, block_cols, block_bytes)
    return _cmc_map(first, nhit, ap, gf.shape[0], max_rank)


def _rank_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, metric='cosine', block_cols=None, block_bytes=None):
    """Per-query (first match rank, #matches, AP) device arrays of rank_metrics_streaming (= grl_rank_metrics's)."""
    nq, ng = qf.shape[0], gf.shape[0]
    lo, hi, sharded = _shard(ng)
    blocks = _ColumnBlocks(qf, gf, metric, block_cols, block_bytes, lo, hi)
    return _rank_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, sharded)


def _rank_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, sharded):
    """The two passes of _rank_streaming over a block source (``_BlockSource``: a block is asked for twice)."""
    import numpy as np
    from . import dist as grl_dist
    dev = blocks.qf.device

    qp, qc = _ids(q_pids, nq, 'q_pids'), _ids(q_camids, nq, 'q_camids')
    gp, gc = _ids(g_pids, ng, 'g_pids'), _ids(g_camids, ng, 'g_camids')
    # pid -> ascending gallery indices (CSR); a query's candidates are its pid's list
    order = np.argsort(gp, kind='stable').astype(np.int32)
    uniq, starts = np.unique(gp[order], return_index=True)
    pid_ptr = np.append(starts, ng).astype(np.int32)
    slot = np.searchsorted(uniq, qp)
    found = slot < uniq.size
    found[found] = uniq[slot[found]] == qp[found]
    q_slot = np.where(found, slot, -1).astype(np.int32)
    cand_len = np.where(found, pid_ptr[np.minimum(slot + 1, uniq.size)] - pid_ptr[np.minimum(slot, uniq.size - 1)], 0)
    cand_off = np.zeros(nq + 1, np.int64)
    np.cumsum(cand_len, out=cand_off[1:])
    total = max(int(cand_off[-1]), 1)

    def dev32(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_qp, t_qc, t_gp, t_gc = dev32(qp), dev32(qc), dev32(gp), dev32(gc)
    t_slot, t_ptr, t_list, t_off = dev32(q_slot), dev32(pid_ptr), dev32(order), dev32(cand_off)
    cand_key = torch.zeros(total, dtype=torch.int32, device=dev)
    one_pass = len(blocks.spans) == 1
    d = None
    for c0, c1 in blocks.spans:
        d = blocks.block(c0, c1)
        _call('grl_match_gather', ptr(d), c1 - c0, nq, c0, c1 - c0, ptr(t_slot), ptr(t_ptr), ptr(t_list), ptr(t_off),
              ptr(cand_key))
    if sharded:
        grl_dist._all_reduce_sum(cand_key)          # each candidate was written by exactly one rank, zero elsewhere
    match_key = torch.empty(total, dtype=torch.int64, device=dev)
    n_match = torch.empty(nq, dtype=torch.int32, device=dev)
    _call('grl_match_sort', nq, ptr(t_slot), ptr(t_ptr), ptr(t_list), ptr(t_qc), ptr(t_gc), ptr(t_off),
          ptr(cand_key), int(cand_len.max()) if nq else 0, ptr(match_key), ptr(n_match))
    max_match = int(n_match.max().item())
    hist = torch.zeros(total, dtype=torch.int32, device=dev)
    if max_match > 0:
        for c0, c1 in blocks.spans:
            if not one_pass:
                d = blocks.block(c0, c1)
            _call('grl_rank_count_block', ptr(d), c1 - c0, nq, c0, c1 - c0, ptr(t_qp), ptr(t_gp), ptr(t_off),
                  ptr(match_key), ptr(n_match), max_match, ptr(hist))
    if sharded:
        grl_dist._all_reduce_sum(hist)
    first = torch.empty(nq, dtype=torch.int32, device=dev)
    nhit = torch.empty(nq, dtype=torch.int32, device=dev)
    ap = torch.empty(nq, dtype=torch.float64, device=dev)
    _call('grl_rank_finish', nq, ptr(t_off), ptr(n_match), ptr(hist), ptr(first), ptr(nhit), ptr(ap))
    return first, nhit, ap


# ----------------------------------------------------------------------------
# pair-level (verification) metrics: ROC, AUC, EER, TPR@FPR over column blocks (roc.hip)
# ----------------------------------------------------------------------------
ROC_BITS_MIN, ROC_BITS_MAX, ROC_BITS_DEFAULT = 8, 20, 16
ROC_FPR_TARGETS = (1e-4, 1e-3, 1e-2, 1e-1)


def _roc_bits(bits, what):
    return _int_arg(bits, ROC_BITS_MIN, ROC_BITS_MAX, what, 'bits')


class PairRoc(object):
    """The verification metrics of a set of (query, gallery) pair distances (lower = more alike), from two histograms
    over the order-preserving uint32 key of the float32 distance, bin = key >> (32 - bits):

      pos, neg     int64 device tensors [2^bits]: same pid from another camera / another pid (same pid AND camera is
                   dropped, the junk rule of eva_functions.evaluate).  Integer counts: independent of block width,
                   summation order and sharding.
      n_pos, n_neg their sums (ValueError at construction if either is 0, saying which)
      auc          Mann-Whitney: P(a positive's bin < a negative's bin) + 0.5 P(same bin), float64
      auc_slack    0.5 sum_b pos_b neg_b / (n_pos n_neg): |auc - AUC of the unquantised distances| is at most this,
                   because only pairs that share a bin can be ordered differently
      eer          bins are accepted in ascending order; at the first bin boundary where FPR >= 1 - TPR, the FPR
                   linearly interpolated (in FPR + TPR - 1) between that boundary and the one before it
      eer_threshold  the threshold (float32, as in curve()) of that first boundary
      tpr_at_fpr(f)  TPR at the last boundary whose FPR <= f
      curve()      (fpr, tpr, threshold) float64 / float64 / float32 numpy arrays over the non-empty bins: the rates
                   after accepting the bin, and the bin's upper edge (accept d <= threshold).  The bin that holds
                   +inf ends at +inf; a bin above it holds NaN keys only (the last bin, for bits >= 9) and its
                   threshold is NaN: NaN distances are accepted last

    For a ``verify_metric`` with beta = 1 the distance is the head's negated logit difference, so
    ``verify_prob(threshold)`` is the pair probability P(same) at which a threshold accepts."""

    def __init__(self, pos, neg, bits):
        self.pos, self.neg, self.bits = pos, neg, bits
        self.n_pos, self.n_neg = (int(v) for v in torch.stack((pos.sum(), neg.sum())).tolist())
        if self.n_pos == 0 or self.n_neg == 0:
            raise ValueError('pair ROC: no %s pairs (n_pos = %d, n_neg = %d): %s'
                             % ('positive' if self.n_pos == 0 else 'negative', self.n_pos, self.n_neg,
                                'no query has a gallery entry of its pid from another camera' if self.n_pos == 0
                                else 'every gallery entry shares the pid of every query'))
        self._pts = None

    def _points(self):
        """(bin ids, pos, neg, tpr, fpr) over the non-empty bins; the rates are those after accepting the bin."""
        if self._pts is None:
            import numpy as np
            p, n = self.pos.cpu().numpy(), self.neg.cpu().numpy()
            b = np.flatnonzero((p != 0) | (n != 0))
            p, n = p[b], n[b]
            self._pts = (b, p, n, np.cumsum(p) / float(self.n_pos), np.cumsum(n) / float(self.n_neg))
        return self._pts

    @property
    def auc(self):
        import numpy as np
        _, p, n, _, _ = self._points()
        above = self.n_neg - np.cumsum(n)                  # negatives in higher bins
        return float((p.astype(np.float64) * (above + 0.5 * n)).sum() / (float(self.n_pos) * float(self.n_neg)))

    @property
    def auc_slack(self):
        import numpy as np
        _, p, n, _, _ = self._points()
        return float(0.5 * (p.astype(np.float64) * n).sum() / (float(self.n_pos) * float(self.n_neg)))

    @property
    def eer(self):
        import numpy as np
        _, _, _, tpr, fpr = self._points()
        f = fpr + tpr - 1.0                                # < 0 at the boundary before the first bin, 1 after the last
        k = int(np.argmax(f >= 0.0))
        f0, fpr0 = (f[k - 1], fpr[k - 1]) if k > 0 else (-1.0, 0.0)
        return float(fpr0 + (0.0 - f0) / (f[k] - f0) * (fpr[k] - fpr0))

    @property
    def eer_threshold(self):
        """The ``curve()`` threshold (float32) of the bin boundary ``eer`` selects, the first where FPR >= 1 - TPR:
        accepting d <= eer_threshold is the operating point next to the equal error rate (``cluster``'s eps)."""
        import numpy as np
        _, _, _, tpr, fpr = self._points()
        return self.curve()[2][int(np.argmax(fpr + tpr - 1.0 >= 0.0))]

    def tpr_at_fpr(self, target):
        import numpy as np
        _, _, _, tpr, fpr = self._points()
        k = int(np.searchsorted(fpr, float(target), side='right'))
        return float(tpr[k - 1]) if k > 0 else 0.0

    def curve(self):
        import numpy as np
        b, _, _, tpr, fpr = self._points()
        shift = np.uint64(32 - self.bits)
        lower, key = b.astype(np.uint64) << shift, ((b.astype(np.uint64) + 1) << shift) - 1
        inf_key = np.uint64(0xff800000)                # the keys above +inf are NaN patterns: the bin that holds +inf
        key = np.where((key > inf_key) & (lower <= inf_key), inf_key, key).astype(np.uint32)       # ends at +inf
        u = np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32)
        return fpr, tpr, u.view(np.float32)

    def summary(self):
        """The scalar figures as a dict of plain Python numbers (what the evaluator prints and stores)."""
        return {'bits': self.bits, 'n_pos': self.n_pos, 'n_neg': self.n_neg, 'auc': self.auc,
                'auc_slack': self.auc_slack, 'eer': self.eer,
                'tpr_at_fpr': {'%g' % f: self.tpr_at_fpr(f) for f in ROC_FPR_TARGETS}}


def _pair_hist_block(d, c0, ids, bits, pos, neg):
    """One grl_pair_hist_block launch: the block d [nq, ncols] (rows strided by d.stride(0), gallery entries c0 ..)
    added to pos / neg."""
    nq, ncols = d.shape
    _call('grl_pair_hist_block', ptr(d), d.stride(0), nq, c0, ncols, ptr(ids[0]), ptr(ids[1]), ptr(ids[2]),
          ptr(ids[3]), bits, ptr(pos), ptr(neg))


def _roc_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, bits, sharded):
    """The histogram pass of pair_roc over a block source (``_BlockSource``): one block, one launch.  Under sharding every rank has counted its own gallery columns; the sum is the whole."""
    bits = _roc_bits(bits, 'pair ROC')
    dev = blocks.qf.device
    ids = (_ids(q_pids, nq, 'q_pids', dev), _ids(q_camids, nq, 'q_camids', dev), _ids(g_pids, ng, 'g_pids', dev),
           _ids(g_camids, ng, 'g_camids', dev))
    hist = torch.zeros((2, 1 << bits), dtype=torch.int64, device=dev)
    if nq:
        for c0, c1 in blocks.spans:
            _pair_hist_block(blocks.block(c0, c1), c0, ids, bits, hist[0], hist[1])
    if sharded:
        from . import dist as grl_dist
        grl_dist._all_reduce_sum(hist)
    return PairRoc(hist[0], hist[1], bits)


def pair_roc(qf, gf, q_pids, g_pids, q_camids, g_camids, metric='cosine', bits=ROC_BITS_DEFAULT, block_cols=None,
             block_bytes=None):
    """ROC / AUC / EER / TPR@FPR of all (query, gallery) pairs under ``metric`` ('cosine', 'euclidean' or a
    ``verify_metric``) as a ``PairRoc``, without the query x gallery matrix: CMC and mAP look at the order inside a
    query's row, this asks whether ONE threshold separates same-identity from different-identity pairs.  The column
    blocks are those of ``search`` and ``rank_metrics_streaming`` (same bits as the full matrix); each is read once by
    grl_pair_hist_block, which classifies the entries by the id arrays (no nq x ng mask) and counts them in two
    int64 histograms of 2^bits bins (8 <= bits <= 20).  The host receives those two arrays, whatever nq x ng is.
    Under torch.distributed the gallery rows are sharded over the ranks and the histograms are all-reduced (integer
    sums: bit-equal to one process); every rank returns the full result.  ValueError: bad ``bits``, id lists of the
    wrong length, no positive or no negative pair."""
    bits = _roc_bits(bits, 'pair_roc')
    nq, ng = qf.shape[0], gf.shape[0]
    lo, hi, sharded = _shard(ng)
    blocks = _ColumnBlocks(qf, gf, metric, block_cols, block_bytes, lo, hi)
    return _roc_blocks(blocks, nq, ng, q_pids, g_pids, q_camids, g_camids, bits, sharded)


def pair_roc_matrix(distmat, q_pids, g_pids, q_camids, g_camids, bits=ROC_BITS_DEFAULT):
    """``pair_roc`` of a [nq, ng] float32 distance matrix that already lives on the device (cosin_dist, verify_dist,
    the device re_ranking's result); rows may be strided (a column slice of a wider matrix is read in place).  Not
    collective: every rank that holds the matrix gets the result from it."""
    bits = _roc_bits(bits, 'pair_roc_matrix')
    require_device(distmat, 'distmat')
    if distmat.dim() != 2:
        raise ValueError('pair_roc_matrix: distmat must be [nq, ng] (got %s)' % (tuple(distmat.shape),))
    nq, ng = distmat.shape
    if nq and ng and (distmat.stride(1) != 1 or distmat.stride(0) < ng):
        distmat = distmat.contiguous()


    class _Whole(object):                           # a block source of one block: the matrix itself
        spans = [(0, ng)] if ng else []
        qf = distmat

        @staticmethod
        def block(c0, c1):
            return distmat
    return _roc_blocks(_Whole, nq, ng, q_pids, g_pids, q_camids, g_camids, bits, False)


# ----------------------------------------------------------------------------
# identity discovery: DBSCAN on the eps-graph of the distance GEMM's column blocks (cluster.hip)
# ----------------------------------------------------------------------------
CLUSTER_MAX_EDGES = int(os.environ.get('GRL_CLUSTER_MAX_EDGES', str(1 << 28)))    # col is int32 [E]: 1 GiB at the limit
CLUSTER_ROUND_BATCH = 4                    # component rounds enqueued per read-back of their "changed" flags


def _cluster_eps(eps, what):
    """eps as the float32 the kernel compares with (a Python float; +inf stays +inf and means FLT_MAX there)."""
    import numpy as np
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or eps != eps:
        raise ValueError('%s: eps must be a number and not NaN (got %r)' % (what, eps))
    with np.errstate(over='ignore'):
        return float(np.float32(eps))


def _cluster_min_samples(m, what):
    return _int_arg(m, 1, _INT_MAX, what, 'min_samples', '>= 1')


class Clustering(object):
    """The result of ``cluster`` / ``cluster_matrix`` / ``cluster_from_graph`` (DBSCAN):

      labels       int64 device [n]: cluster id 0, 1, .. in ascending order of each cluster's smallest core index; -1 = noise
      core         bool device [n]: deg + 1 >= min_samples
      parent       int32 device [n]: a core point's root (its cluster's smallest core index); i for a non-core point
      n_clusters, n_noise, n_edges (stored directed edges E), rounds (component rounds run), eps, min_samples
      pair_scores(pids)   pairwise precision / recall / F1 / ARI of the labels against true identities
      centroids(xf, reduce='unit')   the clusters' centres (cluster_centroids)
      silhouette(xf, metric='cosine', noise='singleton')   the label-free score of the labels (silhouette)"""

    def __init__(self, labels, core, parent, n_clusters, n_noise, n_edges, rounds, eps, min_samples):
        self.labels, self.core, self.parent = labels, core, parent
        self.n_clusters, self.n_noise, self.n_edges, self.rounds = n_clusters, n_noise, n_edges, rounds
        self.eps, self.min_samples = eps, min_samples

    def pair_scores(self, pids):
        """Pair-counting scores of the labels against ``pids`` [n], on the host over the n labels; a noise point is a
        cluster of its own.  With the contingency table of (cluster, pid): tp = sum over cells of C(count, 2),
        pred_pairs = sum over clusters, true_pairs = sum over pids, total_pairs = C(n, 2) (Python ints).
        precision = tp / pred_pairs (1.0 when nothing is predicted together), recall = tp / true_pairs (1.0 when no
        two samples share a pid), f1 = their harmonic mean (0.0 when both are 0), ari = the adjusted Rand index in
        its pair-count form 2 (tp tn - fp fn) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)), 1.0 when fp = fn = 0.
        All four are float64."""
        return _pair_scores(self.labels, self.n_clusters, pids)

    def centroids(self, xf, reduce='unit'):
        """The clusters' centres ``(centroids [n_clusters, d], counts int64 [n_clusters])`` of the rows of ``xf`` the
        labels were computed from: ``cluster_centroids(xf, labels, n_clusters, reduce)``, noise ignored."""
        return cluster_centroids(xf, self.labels, self.n_clusters, reduce)

    def silhouette(self, xf, metric='cosine', noise='singleton'):
        """``silhouette(xf, labels, metric, noise)`` of the rows the labels were computed from."""
        return silhouette(xf, self.labels, metric, noise)


def _pair_scores(labels, n_clusters, pids):
    """``Clustering.pair_scores`` / ``KMeans.pair_scores``: ``labels`` int64 device [n]; a label < 0 (noise, an
    unassigned sample) is a cluster of its own, numbered from ``n_clusters``."""
    import numpy as np
    lab = labels.cpu().numpy().astype(np.int64)
    n = lab.size
    pids = np.asarray(pids).reshape(-1)
    if pids.size != n:
        raise ValueError('pair_scores: expected %d pids, got %d' % (n, pids.size))
    noise = lab < 0
    lab[noise] = n_clusters + np.arange(int(noise.sum()))

    def pairs(counts):
        counts = counts.astype(np.int64)
        return int((counts * (counts - 1) // 2).sum())
    tp = pred = true = 0
    if n:
        pi = np.unique(pids, return_inverse=True)[1].reshape(-1).astype(np.int64)
        tp = pairs(np.unique(lab * (int(pi.max()) + 1) + pi, return_counts=True)[1])
        pred = pairs(np.unique(lab, return_counts=True)[1])
        true = pairs(np.unique(pi, return_counts=True)[1])
    total = n * (n - 1) // 2
    fp, fn = pred - tp, true - tp
    tn = total - tp - fp - fn
    precision = tp / pred if pred else 1.0
    recall = tp / true if true else 1.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fp * fn) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return {'precision': float(precision), 'recall': float(recall), 'f1': float(f1), 'ari': float(ari), 'tp': tp,
            'pred_pairs': pred, 'true_pairs': true, 'total_pairs': total, 'n': n}


def _eps_graph_blocks(blocks, n, eps, max_edges=None):
    """``eps_graph`` over any block source (``_BlockSource``) of the n x n distance matrix, asked for twice: count pass, grl_rrs_scan, one read-back of E = row_ptr[n], fill pass."""
    eps = _cluster_eps(eps, 'eps_graph')
    limit = CLUSTER_MAX_EDGES if max_edges is None else int(max_edges)
    dev = blocks.qf.device
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n == 0:
        return row_ptr, torch.empty(0, dtype=torch.int32, device=dev)

    def sweep(rp, col):
        for c0, c1 in blocks.spans:
            d = blocks.block(c0, c1)
            _call('grl_cluster_edges_block', ptr(d), d.stride(0), n, 0, c0, c1 - c0, eps, ptr(cnt), rp, col)
    sweep(None, None)
    _call('grl_rrs_scan', ptr(cnt), n, ptr(row_ptr))
    n_edges = int(row_ptr[n])
    if n_edges > limit:
        raise ValueError('eps_graph: eps = %r gives E = %d edges among %d samples, more than the limit of %d '
                         '(max_edges / GRL_CLUSTER_MAX_EDGES): lower eps or raise the limit' % (eps, n_edges, n, limit))
    col = torch.empty(n_edges, dtype=torch.int32, device=dev)
    if n_edges:
        cnt.zero_()
        sweep(ptr(row_ptr), ptr(col))
    return row_ptr, col


def _cluster_metric(metric, what):
    if isinstance(metric, VerifyMetric):
        raise ValueError('%s: a verify_metric is the signed logit of modified query rows against gallery rows, not a '
                         "distance between two samples of one set; cluster by 'cosine' or 'euclidean'" % what)
    if metric not in ('cosine', 'euclidean'):
        raise ValueError("%s: metric must be 'cosine' or 'euclidean' (got %r)" % (what, metric))


def eps_graph(xf, eps, metric='cosine', block_cols=None, block_bytes=None, max_edges=None):
    """The eps-neighbourhood graph of the rows of ``xf`` as a CSR ``(row_ptr int64 [n+1], col int32 [E])`` on the
    device, without the n x n matrix: edge i -> j (j != i) iff D[i][j] <= float32(eps), D = ``cosin_dist(xf, xf)``
    ('cosine': eps is a negated dot product, e.g. -0.7, the unit of roc.json's thresholds) or
    ``pairwise_distance_tensor(xf, xf)`` ('euclidean').  A NaN distance is no edge; eps = +inf means FLT_MAX.  The
    column blocks are ``search``'s (the full matrix's bits) and are computed twice: a count pass, one read-back of E, a
    fill pass.  Columns ascend in every row; the result is the same bit for bit on every run and for every block width.
    ValueError: a NaN eps, a ``verify_metric``, E above ``max_edges`` (default GRL_CLUSTER_MAX_EDGES = 2^28) -- raised
    before ``col`` is allocated.  Not sharded: under torch.distributed every rank computes the full, identical graph."""
    _cluster_metric(metric, 'eps_graph')
    eps = _cluster_eps(eps, 'eps_graph')
    require_device(xf, 'xf')
    if xf.shape[0] == 0:                   # (no rows: no feature size to infer, nothing to compute)
        return (torch.zeros(1, dtype=torch.int64, device=xf.device), torch.empty(0, dtype=torch.int32, device=xf.device))
    blocks = _ColumnBlocks(xf, xf, metric, block_cols, block_bytes)
    return _eps_graph_blocks(blocks, blocks.nq, eps, max_edges)


def cluster_from_graph(row_ptr, col, n, min_samples=1, eps=None, _checked=False):
    """DBSCAN's labels from a neighbourhood graph in CSR form on the device (``row_ptr`` int64 [n+1], ``col`` int32
    [E]; any order inside a row): deg[i] = the stored entries of row i, core iff deg + 1 >= min_samples, i ~ j iff
    i -> j or j -> i is stored, clusters = the connected components of the core points under ~, numbered in ascending
    order of their smallest core index; a non-core point next to a core takes the smallest id among its adjacent
    cores, everything else is noise (-1).  The components come from rounds of hooking (integer atomicMin) and pointer
    jumping; the host reads one flag word per ``CLUSTER_ROUND_BATCH`` rounds and raises RuntimeError beyond n + 1
    rounds.  ``eps`` is only recorded.  Not sharded: every rank computes the full result.  ValueError: a malformed
    CSR, a bool or non-integer ``min_samples``."""
    min_samples = _cluster_min_samples(min_samples, 'cluster_from_graph')
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError('cluster_from_graph: n must be an integer >= 0 (got %r)' % (n,))
    n = int(n)
    for t, dt, what in ((row_ptr, torch.int64, 'row_ptr'), (col, torch.int32, 'col')):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 1):
            raise ValueError('cluster_from_graph: %s must be a 1-d %s device tensor' % (what, dt))
    if row_ptr.numel() != n + 1:
        raise ValueError('cluster_from_graph: row_ptr must have n + 1 = %d entries (got %d)' % (n + 1, row_ptr.numel()))
    row_ptr, col = row_ptr.contiguous(), col.contiguous()
    dev, n_edges = row_ptr.device, col.numel()
    length = row_ptr[1:] - row_ptr[:-1]
    if not _checked:                       # a caller's graph: the kernels index parent / core by col
        bad = torch.stack((row_ptr[0] != 0, row_ptr[n] != n_edges,
                           (length < 0).any() if n else row_ptr[0] != 0,
                           ((col < 0) | (col >= n)).any() if n_edges else row_ptr[0] != 0)).tolist()
        if any(bad):
            raise ValueError('cluster_from_graph: malformed CSR (%s)' % ', '.join(
                w for w, b in zip(('row_ptr[0] != 0', 'row_ptr[n] != len(col)', 'row_ptr descends',
                                   'a column outside 0..n-1'), bad) if b))
    deg = length.to(torch.int32)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    border = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return Clustering(labels, core.bool(), parent, 0, 0, 0, 0, eps, min_samples)
    _call('grl_cluster_init', ptr(deg), n, min_samples, ptr(core), ptr(parent), ptr(border))
    flags = torch.empty(CLUSTER_ROUND_BATCH, dtype=torch.int32, device=dev)
    rounds, cap, done = 0, n + 1, False
    while not done:
        if rounds >= cap:
            raise RuntimeError('cluster_from_graph: the components did not settle in %d rounds' % cap)
        batch = min(CLUSTER_ROUND_BATCH, cap - rounds)
        flags.zero_()
        for r in range(batch):
            _call('grl_cluster_round', ptr(row_ptr), ptr(col), ptr(core), ptr(parent), n, flags.data_ptr() + 4 * r)
        changed = flags[:batch].tolist()                 # one read-back per batch
        quiet = changed.index(0) if 0 in changed else -1
        rounds += batch if quiet < 0 else quiet + 1      # rounds after the first quiet one changed nothing
        done = quiet >= 0
    _call('grl_cluster_border', ptr(row_ptr), ptr(col), ptr(core), ptr(parent), n, ptr(border))
    is_root = torch.empty(n, dtype=torch.int32, device=dev)
    root_id = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _call('grl_cluster_roots', ptr(core), ptr(parent), n, ptr(is_root))
    _call('grl_rrs_scan', ptr(is_root), n, ptr(root_id))
    _call('grl_cluster_labels', ptr(core), ptr(parent), ptr(border), ptr(root_id), n, ptr(labels))
    n_clusters, n_noise = torch.stack((root_id[n], (labels < 0).sum())).tolist()
    return Clustering(labels, core.bool(), parent, int(n_clusters), int(n_noise), n_edges, rounds, eps, min_samples)


def cluster(xf, eps, min_samples=1, metric='cosine', block_cols=None, block_bytes=None, max_edges=None):
    """DBSCAN of the rows of ``xf`` at the threshold ``eps`` on the project's own distance ('cosine' = cosin_dist,
    eps a negated dot product such as ``PairRoc.eer_threshold``; 'euclidean' = pairwise_distance_tensor):
    ``cluster_from_graph(*eps_graph(xf, eps, metric, ...), n, min_samples)`` as a ``Clustering``.  For a symmetric
    distance the labels and the core set are those of sklearn's DBSCAN(metric='precomputed'); min_samples = 1 is plain
    threshold linkage, 2 turns singletons into noise.  The host never holds more than the n labels.  Not sharded:
    under torch.distributed every rank computes the full, identical result."""
    min_samples = _cluster_min_samples(min_samples, 'cluster')
    eps = _cluster_eps(eps, 'cluster')
    row_ptr, col = eps_graph(xf, eps, metric, block_cols, block_bytes, max_edges)
    return cluster_from_graph(row_ptr, col, xf.shape[0], min_samples, eps=eps, _checked=True)


def cluster_matrix(distmat, eps, min_samples=1, max_edges=None):
    """``cluster`` on an [n, n] float32 distance matrix that already lives on the device (any square matrix a caller
    can build; it need not be symmetric: i ~ j iff either entry passes); rows may be strided (a column slice of a
    wider matrix is read in place).  ValueError: not square.  Not collective: every rank that holds the matrix
    gets the result from it."""
    min_samples = _cluster_min_samples(min_samples, 'cluster_matrix')
    eps = _cluster_eps(eps, 'cluster_matrix')
    require_device(distmat, 'distmat')
    if distmat.dim() != 2 or distmat.shape[0] != distmat.shape[1]:
        raise ValueError('cluster_matrix: distmat must be square [n, n] (got %s)' % (tuple(distmat.shape),))
    n = distmat.shape[0]
    if n and (distmat.stride(1) != 1 or distmat.stride(0) < n):
        distmat = distmat.contiguous()

    class _Whole(object):                           # a block source of one block: the matrix itself
        spans = [(0, n)] if n else []
        qf = distmat

        @staticmethod
        def block(c0, c1):
            return distmat
    row_ptr, col = _eps_graph_blocks(_Whole, n, eps, max_edges)
    return cluster_from_graph(row_ptr, col, n, min_samples, eps=eps, _checked=True)


# ----------------------------------------------------------------------------
# k-means and cluster centroids: search's top-1 assignment + a deterministic segmented row sum (kmeans.hip)
# ----------------------------------------------------------------------------
KMEANS_REDUCE = {'sum': 0, 'mean': 1, 'unit': 2}         # GRL_KMEANS_SUM / _MEAN / _UNIT of include/grl_hip.h


def _kmeans_int(v, lo, what, name):
    return _int_arg(v, lo, _INT_MAX, what, name, '>= %d' % lo)


def _kmeans_rows(xf, what):
    require_device(xf, 'xf')
    if xf.dim() < 2:
        raise ValueError('%s: xf must be [n, d] (got %s)' % (what, tuple(xf.shape)))
    xf = xf.contiguous().view(xf.shape[0], -1)
    if xf.shape[1] == 0:
        raise ValueError('%s: xf has no feature columns' % what)
    return xf


def _kmeans_top1(xf, centroids, metric, block_cols, block_bytes):
    """The k = 1 running lists of ``search(xf, centroids, 1, metric)`` as the kernels keep them: ``run_key`` int64 [n]
    (the composites) and ``run_val`` float32 [n].  Unsharded: every rank assigns every sample."""
    blocks = _ColumnBlocks(xf, centroids, metric, block_cols, block_bytes)
    n = blocks.nq
    top = _TopK(n, 1, xf.device)
    if n:
        for c0, c1 in blocks.spans:
            top.push(blocks.block(c0, c1), c1 - c0, c1 - c0, c0)
    return top.key.view(n), top.val.view(n)


def _kmeans_relabel(run_key, run_val, k, prev_labels=None):
    """(labels int32 [n], counts int32 [k], changed int32 [1]) of a top-1 assignment (grl_kmeans_relabel)."""
    n, dev = run_key.shape[0], run_key.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(k, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    _call('grl_kmeans_relabel', ptr(run_key), ptr(run_val), n, k, ptr(prev_labels), ptr(labels), ptr(counts),
          ptr(changed))
    return labels, counts, changed


def _kmeans_update(xf, labels32, counts32, k, reduce, prev=None):
    """Centroids [k, d] of int32 labels (< 0 or >= k: nobody's) whose per-cluster counts are ``counts32``: member
    lists, the segmented row sum, the finish.  Returns ``(centroids, empty int32 [1])``; nothing is read back."""
    n, d = xf.shape
    dev = xf.device
    mptr = torch.empty(k + 1, dtype=torch.int64, device=dev)
    _call('grl_rrs_scan', ptr(counts32), k, ptr(mptr))
    cursor = torch.zeros(k, dtype=torch.int32, device=dev)
    tmp = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    mem = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _call('grl_kmeans_members', ptr(labels32), n, k, ptr(mptr), ptr(cursor), ptr(tmp), ptr(mem))
    lds = (d + 3) // 4 * 4                            # rows grl_row_sqnorm can read; the padding stays zero
    total = torch.zeros((k, lds), dtype=torch.float32, device=dev)
    _call('grl_segment_rowsum', ptr(xf), xf.stride(0), n, ptr(mptr), ptr(mem), n, k, d, ptr(total), lds)
    sq = None
    if reduce == 'unit':
        sq = torch.empty(k, dtype=torch.float32, device=dev)
        _call('grl_row_sqnorm', ptr(total), ptr(sq), k, lds, lds)
    out = torch.empty((k, d), dtype=torch.float32, device=dev)
    empty = torch.zeros(1, dtype=torch.int32, device=dev)
    _call('grl_kmeans_finish', ptr(total), lds, ptr(counts32), ptr(sq), ptr(prev), prev.stride(0) if prev is not None else 0,
          k, d, KMEANS_REDUCE[reduce], ptr(out), d, ptr(empty))
    return out, empty


def _kmeans_prev(prev, k, d, what):
    if prev is None:
        return None
    require_device(prev, 'prev')
    if tuple(prev.shape) != (k, d):
        raise ValueError('%s: prev must be [k, d] = [%d, %d] (got %s)' % (what, k, d, tuple(prev.shape)))
    return prev.contiguous()


def kmeans_assign(xf, centroids, metric='cosine', block_cols=None, block_bytes=None):
    """Every sample's nearest centroid: ``(labels int64 [n], dist float32 [n])`` on the device, the index and the
    distance of ``search(xf, centroids, 1, metric)`` bit for bit ('cosine' = cosin_dist, 'euclidean' =
    pairwise_distance_tensor; ties go to the smaller centroid index), except that a sample whose best distance is NaN
    gets label -1 (cosin_dist keeps a NaN; pairwise_distance_tensor's clamp at 1e-12 turns one into a number, which is
    ranked as search ranks it).  The distances are computed in column blocks of the centroids (``block_cols`` / ``block_bytes`` as
    in ``search``): never an [n, k] matrix beyond a block.  Not sharded: every rank assigns every sample.
    ValueError: a ``verify_metric``, no centroid."""
    _cluster_metric(metric, 'kmeans_assign')
    xf = _kmeans_rows(xf, 'kmeans_assign')
    require_device(centroids, 'centroids')
    k = centroids.shape[0]
    if k < 1:
        raise ValueError('kmeans_assign: at least one centroid is needed (got %s)' % (tuple(centroids.shape),))
    run_key, run_val = _kmeans_top1(xf, centroids, metric, block_cols, block_bytes)
    labels = _kmeans_relabel(run_key, run_val, k)[0]
    return labels.to(torch.int64), run_val


def cluster_centroids(xf, labels, k=None, reduce='mean', prev=None):
    """Per-cluster sums / means / unit means of the rows of ``xf`` [n, d]: ``(centroids float32 [k, d], counts int64
    [k])`` on the device.  ``labels``: any integer device tensor [n]; entries < 0 belong to nobody.  ``k`` defaults to
    max(label) + 1.  Cluster j's members are summed in a fixed order (ascending sample index dealt to four partial
    sums), without floating-point atomics: the same bits on every run, unlike ``index_add_``.
    ``reduce``: 'sum', 'mean' (sum / count) or 'unit' (sum scaled to unit length).  A cluster without members -- or,
    for 'unit', with a sum whose norm is zero or not finite -- takes its row of ``prev`` [k, d] when given, else zeros.
    ValueError: a label >= k (one device-side check), labels that are not n integers, an unknown ``reduce``."""
    xf = _kmeans_rows(xf, 'cluster_centroids')
    n, d = xf.shape
    if reduce not in KMEANS_REDUCE:
        raise ValueError("cluster_centroids: reduce must be 'sum', 'mean' or 'unit' (got %r)" % (reduce,))
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dim() == 1 and labels.numel() == n
            and not labels.dtype.is_floating_point and not labels.dtype.is_complex and labels.dtype != torch.bool):
        raise ValueError('cluster_centroids: labels must be an integer device tensor with one entry per row of xf '
                         '(%d)' % n)
    top = int(labels.max()) if n else -1              # the one read-back: k's default and the bound check
    k = _kmeans_int(max(top + 1, 0) if k is None else k, 0, 'cluster_centroids', 'k')
    if top >= k:
        raise ValueError('cluster_centroids: label %d is outside 0..k-1 = 0..%d' % (top, k - 1))
    prev = _kmeans_prev(prev, k, d, 'cluster_centroids')
    if k == 0:
        return (torch.empty((0, d), dtype=torch.float32, device=xf.device),
                torch.empty(0, dtype=torch.int64, device=xf.device))
    labels32 = labels.to(torch.int64).clamp(min=-1).to(torch.int32)
    counts = torch.zeros(k, dtype=torch.int32, device=xf.device)
    _call('grl_kmeans_label_counts', ptr(labels32), n, k, ptr(counts))
    out, _ = _kmeans_update(xf, labels32, counts, k, reduce, prev)
    return out, counts.to(torch.int64)


class KMeans(object):
    """The result of ``kmeans``:

      labels       int64 device [n]: the cluster of every sample at the last assignment; -1 = unassigned (a NaN distance)
      centroids    float32 device [k, d]: the update of those labels (``cluster_centroids(xf, labels, k, ..)``)
      counts       int64 device [k]: members per cluster
      n_iter, converged, n_changed (labels changed per iteration; the first entry is n), n_empty (clusters without a
      usable sum at the last update: they kept their previous row), n_unassigned, k, metric
      inertia      float64: the sum over assigned samples of the distance to their centroid at the last assignment
                   ('cosine': the negated dot products; 'euclidean': the squared distances)
      pair_scores(pids)   pairwise precision / recall / F1 / ARI of the labels against true identities
      silhouette(xf, metric=None)   the label-free score of the labels (silhouette)"""

    def __init__(self, labels, centroids, counts, n_iter, converged, n_changed, n_empty, n_unassigned, k, metric,
                 inertia):
        self.labels, self.centroids, self.counts = labels, centroids, counts
        self.n_iter, self.converged, self.n_changed = n_iter, converged, n_changed
        self.n_empty, self.n_unassigned, self.k, self.metric, self.inertia = n_empty, n_unassigned, k, metric, inertia

    def pair_scores(self, pids):
        """``Clustering.pair_scores``: an unassigned sample is a cluster of its own."""
        return _pair_scores(self.labels, self.k, pids)

    def silhouette(self, xf, metric=None):
        """``silhouette(xf, labels, metric)``; ``metric`` defaults to the run's own.  An unassigned
        sample is a cluster of its own, as in ``pair_scores``."""
        return silhouette(xf, self.labels, self.metric if metric is None else metric)


def _kmeans_init(xf, k, init, seed):
    """C0 [k, d] as a fresh device tensor: a [k, d] tensor as it is, k distinct sample indices, or 'random'."""
    import numpy as np
    n, d = xf.shape
    if torch.is_tensor(init) and init.dim() == 2:
        require_device(init, 'init')
        if tuple(init.shape) != (k, d):
            raise ValueError('kmeans: init centroids must be [k, d] = [%d, %d] (got %s)' % (k, d, tuple(init.shape)))
        return init.contiguous().clone()
    if isinstance(init, str):
        if init != 'random':
            raise ValueError("kmeans: init must be 'random', k sample indices or a [k, d] device tensor (got %r)" % (init,))
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError('kmeans: seed must be an integer >= 0 (got %r)' % (seed,))
        idx = np.random.Generator(np.random.PCG64(int(seed))).choice(n, k, replace=False)
    else:
        try:
            idx = np.asarray(init.cpu() if torch.is_tensor(init) else list(init))
        except TypeError:
            raise ValueError("kmeans: init must be 'random', k sample indices or a [k, d] device tensor (got %r)" % (init,))
        if idx.ndim != 1 or idx.dtype.kind not in 'iu' or idx.size != k:
            raise ValueError('kmeans: init must hold k = %d integer sample indices' % k)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError('kmeans: init indices must be in 0..n-1 = 0..%d' % (n - 1))
        if np.unique(idx).size != k:
            raise ValueError('kmeans: init indices must be distinct')
    return xf[torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(xf.device)].contiguous()


def kmeans(xf, k, metric='cosine', init='random', seed=0, max_iter=50, block_cols=None, block_bytes=None):
    """Lloyd's k-means of the rows of ``xf`` [n, d] on the device as a ``KMeans``: 'cosine' is spherical k-means
    (distance = cosin_dist = -dot, centroids = the unit-length sum of the members; the rows and the initial
    centroids should be unit already -- nothing is normalised behind the caller's back), 'euclidean' the classic
    form (pairwise_distance_tensor, centroids = the mean).  Iteration t assigns every sample to its nearest centroid
    (``kmeans_assign``: search's column blocks and tie rule, never an [n, k] matrix beyond a block) and recomputes
    the centroids by the deterministic segmented row sum (``cluster_centroids`` with ``prev`` = the old centroids, so
    an empty cluster keeps its row).  It stops after the first iteration whose labels equal the previous one's
    (``converged``) or after ``max_iter`` iterations; the host reads one int32, the number of changed labels, per
    iteration.  ``init``: a [k, d] device tensor, k distinct sample indices, or 'random' = numpy's
    Generator(PCG64(seed)).choice(n, k, replace=False).  The result is the same bit for bit on every run and for
    every block width.  Not sharded: under torch.distributed every rank computes the full, identical result.
    ValueError: a ``verify_metric``, k outside 1..n, max_iter < 1, a bad ``init``."""
    import numpy as np
    _cluster_metric(metric, 'kmeans')
    xf = _kmeans_rows(xf, 'kmeans')
    n, d = xf.shape
    k = _kmeans_int(k, 1, 'kmeans', 'k')
    if k > n:
        raise ValueError('kmeans: k must be in 1..n = 1..%d (got %d)' % (n, k))
    max_iter = _kmeans_int(max_iter, 1, 'kmeans', 'max_iter')
    cent = _kmeans_init(xf, k, init, seed)
    reduce = 'unit' if metric == 'cosine' else 'mean'
    labels, n_changed, converged = None, [], False
    while len(n_changed) < max_iter and not converged:
        run_key, run_val = _kmeans_top1(xf, cent, metric, block_cols, block_bytes)
        labels, counts, changed = _kmeans_relabel(run_key, run_val, k, labels)
        cent, empty = _kmeans_update(xf, labels, counts, k, reduce, cent)
        n_changed.append(int(changed))                # the iteration's one read-back
        converged = n_changed[-1] == 0
    best = run_val.cpu().numpy().astype(np.float64)
    assigned = labels.cpu().numpy() >= 0
    inertia = float((best[assigned] if metric == 'cosine' else best[assigned] ** 2).sum())
    counts = counts.to(torch.int64)
    return KMeans(labels.to(torch.int64), cent, counts, len(n_changed), converged, n_changed, int(empty),
                  n - int(assigned.sum()), k, metric, inertia)


# ----------------------------------------------------------------------------
# streaming k-reciprocal re-ranking (rerank_stream.hip)
# ----------------------------------------------------------------------------
RERANK_K1_MAX, RERANK_K2_MAX, RERANK_LMAX = 20, 8, 256


class _SampleBlocks(object):
    """Column blocks S[:, i0:i1] of the stacked distance matrix S = [[qq, qg], [qg^T, gg]] over the N = nq + ng
    samples (qq, gg = pairwise_distance_tensor, qg = cosin_dist: what ATTEvaluator hands to re_ranking), as
    SEGMENTS on one side of the query/gallery boundary.  A query segment's lower rows are a row block of qg
    (gemm(qf[i0:i1], gf), read transposed), a gallery segment's come from a column block of gg; every entry has
    the full matrix's bits.  Without ``block_cols`` the width is the multiple of 32 samples whose three buffers
    (upper, lower, D rows) fit ``block_bytes``.  ``lo`` / ``hi`` keep the spans to the samples [lo, hi) (a rank's
    share); the width rule does not look at them, and no entry's bits depend on the spans."""

    def __init__(self, qf, gf, block_cols=None, block_bytes=None, lo=0, hi=None):
        nq, ng = qf.shape[0], gf.shape[0]
        self.nq, self.ng, self.N = nq, ng, nq + ng
        hi = self.N if hi is None else hi
        if block_cols is None:
            block_cols = _sample_block_cols(self.N, block_bytes)
        self.width = w = max(1, min(int(block_cols), hi - lo))
        self.spans = [(i, min(i + w, hi)) for i in range(lo, hi, w)]
        self.qq = _ColumnBlocks(qf, qf, 'euclidean', block_cols=min(w, nq))
        self.qg = _ColumnBlocks(qf, gf, 'cosine', block_cols=min(w, ng))
        self.gg = _ColumnBlocks(gf, gf, 'euclidean', block_cols=min(w, ng))
        self.qf, self.gf = self.qq.qf, self.gg.qf
        self.rows = _new((min(w, nq) * ng,), self.qf)
        self.drows = None

    def segments(self, i0, i1):
        """(s0, s1, up, ldu, lo, lo_rs, lo_cs) for the parts of [i0, i1) left and right of the boundary."""
        nq, ng, k = self.nq, self.ng, self.qf.shape[1]
        if i0 < nq:
            s1 = min(i1, nq)
            n = s1 - i0
            up = self.qq.block(i0, s1)
            lo = self.rows[:n * ng].view(n, ng)
            gemm(self.qf[i0:s1], self.gf, lo, n, ng, k, epilogue=EPI_NEGDOT, math=MATH_F32)
            yield i0, s1, up, n, lo, 1, ng
            i0 = s1
        if i0 < i1:
            n = i1 - i0
            yield i0, i1, self.qg.block(i0 - nq, i1 - nq), n, self.gg.block(i0 - nq, i1 - nq), n, 1

    def d_rows(self, i0, i1, colmax):
        """D[i0:i1, :] of grl_rerank_build ([i1-i0][N] view of a reused buffer); colmax[i0:i1] is filled too."""
        if self.drows is None:
            self.drows = _new((self.width * self.N,), self.qf)
        out = self.drows[:(i1 - i0) * self.N].view(i1 - i0, self.N)
        for s0, s1, up, ldu, lo, lrs, lcs in self.segments(i0, i1):
            _call('grl_rrs_segment_rows', ptr(up), ldu, ptr(lo), lrs, lcs, self.nq, self.ng, s1 - s0,
                  ptr(colmax[s0:]), ptr(out[s0 - i0:]), self.N)
        return out


class _Rerank(object):
    """The sparse state of the k-reciprocal re-ranking of (qf, gf): colmax [N], the first K rank entries of every
    D row, the expansion lists with their weights ([N][256]), V2 as CSR over all samples and the gallery samples'
    V2 as CSC.  Nothing of size N x N or nq x ng is allocated.

    Under torch.distributed (``grl_dist.is_distributed``) rank r of W owns the samples ``shard_rows(N, r, W)``: a
    contiguous range, the first N % W ranks one sample longer.  The passes over the distance GEMM (A1, A2) and the
    expansion run for the owned samples only; colmax, the rank lists, the weights, the row counts and the CSR
    entries are all-gathered in between, each value exactly as its owner wrote it (nothing is reduced), so every
    rank ends with the single-process state, bit for bit."""

    def __init__(self, qf, gf, k1, k2, lambda_value, block_cols=None, block_bytes=None):
        from . import dist as grl_dist
        require_device(qf, 'qf'); require_device(gf, 'gf')
        nq, ng = qf.shape[0], gf.shape[0]
        N = nq + ng
        if qf.dim() != 2 or gf.dim() != 2 or qf.shape[1] != gf.shape[1]:
            raise ValueError('qf [nq, d] and gf [ng, d] must share d (got %s, %s)' % (tuple(qf.shape), tuple(gf.shape)))
        if nq < 1 or ng < 1:
            raise ValueError('re-ranking needs at least one query and one gallery entry')
        if not (1 <= int(k1) <= RERANK_K1_MAX and int(k1) < N):
            raise ValueError('k1 must be in 1..%d and below q + g = %d (got %r)' % (RERANK_K1_MAX, N, k1))
        if not (1 <= int(k2) <= RERANK_K2_MAX and int(k2) <= N):
            raise ValueError('k2 must be in 1..%d and at most q + g = %d (got %r)' % (RERANK_K2_MAX, N, k2))
        self.nq, self.ng, self.N = nq, ng, N
        self.k1, self.k2, self.K = int(k1), int(k2), max(int(k1) + 1, int(k2))
        self.lam, self.one_minus = float(lambda_value), 1 - lambda_value     # float32(1 - lambda), as rerank.py passes it
        self.sharded = sharded = grl_dist.is_distributed()
        rank, world = grl_dist._rank_world(None, None)
        bounds = grl_dist.shard_bounds(N, world)
        lo, hi = bounds[rank], bounds[rank + 1]
        sb = _SampleBlocks(qf, gf, block_cols, block_bytes, lo, hi)
        dev, K = sb.qf.device, self.K
        # pass A1, owned samples: colmax and the first K entries of every D row (grl_row_argsort's order).  A
        # sample's colmax is the maximum over its whole column of S, which its owner holds: gathered, never reduced
        self.colmax = torch.empty(N, dtype=torch.float32, device=dev)
        top = _TopK(hi - lo, K, dev)
        for i0, i1 in sb.spans:
            top.push(sb.d_rows(i0, i1, self.colmax), N, N, 0, rows=(i0 - lo, i1 - lo))
        sb.drows = None
        top.val = None
        self.rank = torch.empty((N, K), dtype=torch.int32, device=dev)
        self.rank[lo:hi] = top.key & 0xffffffff
        del top
        if sharded:
            grl_dist.gather_row_ranges(self.colmax, bounds)
            grl_dist.gather_row_ranges(self.rank, bounds)
        # expansion lists of ALL samples on every rank (a list reads the rank lists of arbitrary samples, so it comes
        # after the gather; one wave per sample, no GEMM), then pass A2 for the owned samples: their weights
        self.lcnt = torch.empty(N, dtype=torch.int32, device=dev)
        self.lidx = torch.empty((N, RERANK_LMAX), dtype=torch.int32, device=dev)
        _call('grl_rrs_lists', ptr(self.rank), K, N, self.k1, ptr(self.lcnt), ptr(self.lidx))
        self.lval = torch.empty((N, RERANK_LMAX), dtype=torch.float32, device=dev)
        for i0, i1 in sb.spans:
            for s0, s1, up, ldu, lo_, lrs, lcs in sb.segments(i0, i1):
                _call('grl_rrs_weights', ptr(up), ldu, ptr(lo_), lrs, lcs, nq, ng, s1 - s0, s0, ptr(self.colmax),
                      ptr(self.lcnt), ptr(self.lidx), ptr(self.lval))
        del sb
        if sharded:
            grl_dist.gather_row_ranges(self.lval, bounds)
        # local query expansion: V2 as CSR.  A counting launch over the owned rows, the counts of all ranks, their
        # prefix sum; the fill then writes the owned rows at their final place and the other ranks' rows follow
        cnt = torch.empty(N, dtype=torch.int32, device=dev)
        _call('grl_rrs_expand_rows', ptr(self.rank), K, ptr(self.lcnt), ptr(self.lidx), ptr(self.lval), N, self.k2, lo,
              hi - lo, None, ptr(cnt), None, None)
        if sharded:
            grl_dist.gather_row_ranges(cnt, bounds)
        self.row_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
        _call('grl_rrs_scan', ptr(cnt), N, ptr(self.row_ptr))
        del cnt
        at = self.row_ptr[torch.tensor(bounds + [nq], device=dev)].tolist()       # the one read-back: sizes to allocate
        nnz, g0 = at[world], at[world + 1]
        self.col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        self.val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        _call('grl_rrs_expand_rows', ptr(self.rank), K, ptr(self.lcnt), ptr(self.lidx), ptr(self.lval), N, self.k2, lo,
              hi - lo, ptr(self.row_ptr), None, ptr(self.col), ptr(self.val))
        if sharded:
            sizes = [at[r + 1] - at[r] for r in range(world)]
            cols = grl_dist.all_gather_uneven(self.col[at[rank]:at[rank + 1]], sizes)
            vals = grl_dist.all_gather_uneven(self.val[at[rank]:at[rank + 1]], sizes)
            for r in range(world):
                if r != rank and sizes[r]:
                    _call('grl_rrs_place', ptr(cols[r]), ptr(vals[r]), sizes[r], ptr(self.row_ptr), bounds[r],
                          bounds[r + 1], ptr(self.col), ptr(self.val))
            del cols, vals
        # inverted index of the gallery samples' rows, ascending j within a column (grl_rrs_final's summation order)
        n_g = max(nnz - g0, 1)
        self.csc_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
        self.csc_row = torch.zeros(n_g, dtype=torch.int32, device=dev)
        self.csc_val = torch.zeros(n_g, dtype=torch.float32, device=dev)
        ccnt = torch.empty(N, dtype=torch.int32, device=dev)
        tmp_row = torch.empty(n_g, dtype=torch.int32, device=dev)
        tmp_val = torch.empty(n_g, dtype=torch.float32, device=dev)
        _call('grl_rrs_transpose', ptr(self.row_ptr), ptr(self.col), ptr(self.val), nq, N, ptr(ccnt), ptr(tmp_row),
              ptr(tmp_val), ptr(self.csc_ptr), ptr(self.csc_row), ptr(self.csc_val))

    def finish(self, d, col0, ncols):
        """d [nq][ncols] (cosin_dist of gallery entries col0 ..) becomes the re-ranked distances, in place."""
        _call('grl_rrs_final', ptr(d), ncols, self.nq, col0, ncols, ptr(self.colmax), ptr(self.row_ptr), ptr(self.col),
              ptr(self.val), ptr(self.csc_ptr), ptr(self.csc_row), ptr(self.csc_val), C.c_float(self.lam),
              C.c_float(self.one_minus))
        return d


class _RerankBlocks(object):
    """Column blocks of the re-ranked q x g distances: cosin_dist blocks transformed in place."""

    def __init__(self, qf, gf, rr, block_cols=None, block_bytes=None):
        if block_cols is None:                      # as _ColumnBlocks, but never the whole q x g matrix in one block
            block_cols = min(_block_cols(rr.nq, block_bytes), max(256, -(-rr.ng // 512) * 256))
        lo, hi, _ = _shard(rr.ng)                   # under torch.distributed: gallery columns sharded as in search
        self.cos = _ColumnBlocks(qf, gf, 'cosine', block_cols, lo=lo, hi=hi)
        self.spans, self.qf, self.rr = self.cos.spans, self.cos.qf, rr

    def block(self, c0, c1):
        return self.rr.finish(self.cos.block(c0, c1), c0, c1 - c0)


def rerank_search(qf, gf, k, k1=20, k2=6, lambda_value=0.3, exclude=None, block_cols=None, block_bytes=None):
    """``search`` on the k-reciprocal re-ranked distances F = re_ranking(cosin_dist(qf, gf), pairwise_distance_tensor(
    qf, qf), pairwise_distance_tensor(gf, gf), k1, k2, lambda_value): ``(dist [nq, k] float32, idx [nq, k] int64)``,
    bit for bit ``rank_rows(F)[:, :k]`` and F at those indices (search's tie, NaN and padding rules), without F, the
    (q+g)^2 matrices or any nq x ng array.  k <= 1024, k1 <= 20, k2 <= 8; no limit on q + g.  Blocks follow
    ``block_cols`` / ``block_bytes`` (GRL_SEARCH_BLOCK_BYTES).  Under torch.distributed the work is sharded over the
    ranks: the sample passes by contiguous sample range with all-gathers of colmax, the rank lists,
    the weights and the V2 rows in between, the final pass by gallery column with search's exchange of top-k
    lists.  Every rank returns the full result, bit for bit the single-process one.

    ``exclude = (q_pids, g_pids, q_camids, g_camids)`` is ``search``'s: row q is ``rank_rows(F)[q]`` with the
    gallery entries of query q's pid AND camera deleted, truncated to ``k``, and F at those indices, bit for bit.
    Only the ranking of the re-ranked blocks is filtered; the K-nearest lists behind the k-reciprocal sets are
    not, as the reference's re_ranking knows nothing of junk, so F itself does not depend on ``exclude``."""
    k = _search_k(k, 'rerank_search')
    junk = _junk_ids(exclude, qf.shape[0], gf.shape[0], qf.device)
    rr = _Rerank(qf, gf, k1, k2, lambda_value, block_cols, block_bytes)
    return _search_blocks(_RerankBlocks(qf, gf, rr, block_cols, block_bytes), rr.nq, k, rr.sharded, junk)


def rerank_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, k1=20, k2=6, lambda_value=0.3, max_rank=100,
                             block_cols=None, block_bytes=None):
    """``rank_metrics(rank_rows(F), ...)`` for the re-ranked distances F of ``rerank_search``: (cmc[max_rank] float32,
    mAP float) with rank_metrics_streaming's contract (first hit and #matches exact, CMC equal, mAP within 1e-12,
    at most 8192 gallery entries per query pid).  Under torch.distributed it is sharded as ``rerank_search`` is, the
    final pass with rank_metrics_streaming's exchange (match keys and rank histograms); first hit, #matches and the
    CMC are the single-process values on every rank, the mAP within the same 1e-12."""
    rr = _Rerank(qf, gf, k1, k2, lambda_value, block_cols, block_bytes)
    return _metrics_from_blocks(_RerankBlocks(qf, gf, rr, block_cols, block_bytes), rr.nq, rr.ng, q_pids, g_pids,
                                q_camids, g_camids, max_rank, rr.sharded)


def rerank_pair_roc(qf, gf, q_pids, g_pids, q_camids, g_camids, k1=20, k2=6, lambda_value=0.3, bits=ROC_BITS_DEFAULT,
                    block_cols=None, block_bytes=None):
    """``pair_roc`` on the k-reciprocal re-ranked distances F of ``rerank_search``: the ``PairRoc`` of
    ``pair_roc_matrix(F, ...)``, bin for bin, without F.  Sharded under torch.distributed as
    ``rerank_metrics_streaming`` is, the final pass with pair_roc's all-reduce of the two histograms."""
    bits = _roc_bits(bits, 'rerank_pair_roc')
    rr = _Rerank(qf, gf, k1, k2, lambda_value, block_cols, block_bytes)
    return _roc_blocks(_RerankBlocks(qf, gf, rr, block_cols, block_bytes), rr.nq, rr.ng, q_pids, g_pids, q_camids,
                       g_camids, bits, rr.sharded)


# ----------------------------------------------------------------------------
# DBSCAN on the k-reciprocal Jaccard distance of one sample set (jaccard.hip)
# ----------------------------------------------------------------------------
def _jaccard_args(xf, eps, k1, k2, what):
    """The checks of ``jaccard_graph`` / ``cluster_jaccard``, all before any device work: (n, eps as the float32 the
    kernel compares with, k1, k2)."""
    import math
    import numpy as np
    if not (torch.is_tensor(xf) and xf.is_cuda and xf.dtype == torch.float32 and xf.dim() == 2):
        raise ValueError('%s: xf must be a 2-d float32 tensor [n, d] on a HIP device (got %s)'
                         % (what, '%s %s on %s' % (tuple(xf.shape), xf.dtype, xf.device) if torch.is_tensor(xf)
                            else type(xf).__name__))
    n = int(xf.shape[0])
    if n < 2 or xf.shape[1] < 1:
        raise ValueError('%s: needs n >= 2 samples of d >= 1 features (got %s)' % (what, tuple(xf.shape)))
    for v, name in ((k1, 'k1'), (k2, 'k2')):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError('%s: %s must be an integer (got %r)' % (what, name, v))
    if not (1 <= k1 <= RERANK_K1_MAX and k1 < n):
        raise ValueError('%s: k1 must be in 1..%d and below n = %d (got %r)' % (what, RERANK_K1_MAX, n, k1))
    if not (1 <= k2 <= RERANK_K2_MAX and k2 <= n):
        raise ValueError('%s: k2 must be in 1..%d and at most n = %d (got %r)' % (what, RERANK_K2_MAX, n, k2))
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real):
        raise ValueError('%s: eps must be a number (got %r)' % (what, eps))
    with np.errstate(over='ignore'):
        e32 = float(np.float32(eps))
    if not math.isfinite(e32) or e32 >= 1.0:
        raise ValueError('%s: eps must be finite and < 1 as a float32 (got %r): at a Jaccard distance of 1 two samples '
                         'share no neighbour, so eps >= 1 joins every pair' % (what, eps))
    return n, e32, int(k1), int(k2)


def _pad_features(xf):
    """``xf`` [n, d] as contiguous rows whose width is a multiple of 32, what the distance GEMM takes: zero columns are
    appended when d is not (they add +0 to every dot product and norm)."""
    n, d = xf.shape
    if d % 32 == 0:
        return xf.contiguous()
    out = torch.zeros((n, -(-d // 32) * 32), dtype=xf.dtype, device=xf.device)
    out[:, :d] = xf
    return out


class _JaccardSet(object):
    """The sparse k-reciprocal state of ONE sample set ``xf`` [n, d] (all-vs-all, nothing stacked, no sample counted
    twice): colmax [n], the first K = max(k1 + 1, k2) rank entries of every D row, the expansion lists with their
    weights ([n][256]), V2 as CSR and its transpose over all rows as CSC.  S = pairwise_distance_tensor(xf, xf) (of the
    rows zero-padded to a multiple of 32 features, ``_pad_features``) comes in column blocks of the 'euclidean' ``_ColumnBlocks`` (twice: pass A1 and pass A2), D[i][j] = S[j][i]^2 / colmax[i];
    the kernels are ``_Rerank``'s, the block [n][w] handed over as one upper row and n - 1 lower rows.  Nothing of size
    n x n is allocated; the block width follows ``_SampleBlocks``' rule.  Not sharded: under torch.distributed every
    rank builds the full, identical state and no collective is issued."""

    def __init__(self, xf, k1, k2, block_cols=None, block_bytes=None):
        n = xf.shape[0]
        self.n, self.k1, self.k2, self.K = n, k1, k2, max(k1 + 1, k2)
        if block_cols is None:
            block_cols = _sample_block_cols(n, block_bytes)
        self.width = w = max(1, min(int(block_cols), n))
        spans = [(i, min(i + w, n)) for i in range(0, n, w)]
        xf = _pad_features(xf)
        cb = _ColumnBlocks(xf, xf, 'euclidean', block_cols=w)
        dev, K = cb.qf.device, self.K

        def segment(i0, i1):                      # S[:, i0:i1] as (up, ldu, lo, lo_rs, lo_cs, nq = 1, ng = n - 1, w)
            s = cb.block(i0, i1)
            return ptr(s), i1 - i0, ptr(s[1:]), i1 - i0, 1, 1, n - 1, i1 - i0
        # pass A1: colmax and the first K entries of every D row (grl_topk_block's order)
        self.colmax = torch.empty(n, dtype=torch.float32, device=dev)
        top = _TopK(n, K, dev)
        drows = _new((w * n,), cb.qf)
        for i0, i1 in spans:
            _call('grl_rrs_segment_rows', *segment(i0, i1) + (ptr(self.colmax[i0:]), ptr(drows), n))
            top.push(drows, n, n, 0, rows=(i0, i1))
        del drows
        top.val = None
        self.rank = (top.key & 0xffffffff).to(torch.int32)
        del top
        # expansion lists, then pass A2: their weights
        self.lcnt = torch.empty(n, dtype=torch.int32, device=dev)
        self.lidx = torch.empty((n, RERANK_LMAX), dtype=torch.int32, device=dev)
        _call('grl_rrs_lists', ptr(self.rank), K, n, k1, ptr(self.lcnt), ptr(self.lidx))
        self.lval = torch.empty((n, RERANK_LMAX), dtype=torch.float32, device=dev)
        for i0, i1 in spans:
            _call('grl_rrs_weights', *segment(i0, i1) + (i0, ptr(self.colmax), ptr(self.lcnt), ptr(self.lidx),
                                                         ptr(self.lval)))
        del cb
        # V2 as CSR (count, scan, one read-back of nnz, fill) and its transpose over all n rows
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        _call('grl_rrs_expand', ptr(self.rank), K, ptr(self.lcnt), ptr(self.lidx), ptr(self.lval), n, k2, None, ptr(cnt),
              None, None)
        self.row_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        _call('grl_rrs_scan', ptr(cnt), n, ptr(self.row_ptr))
        self.nnz = nnz = int(self.row_ptr[n])
        m = max(nnz, 1)
        self.col = torch.empty(m, dtype=torch.int32, device=dev)
        self.val = torch.empty(m, dtype=torch.float32, device=dev)
        _call('grl_rrs_expand', ptr(self.rank), K, ptr(self.lcnt), ptr(self.lidx), ptr(self.lval), n, k2,
              ptr(self.row_ptr), None, ptr(self.col), ptr(self.val))
        self.csc_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.csc_row = torch.zeros(m, dtype=torch.int32, device=dev)
        self.csc_val = torch.zeros(m, dtype=torch.float32, device=dev)
        tmp_row = torch.empty(m, dtype=torch.int32, device=dev)
        tmp_val = torch.empty(m, dtype=torch.float32, device=dev)
        _call('grl_rrs_transpose', ptr(self.row_ptr), ptr(self.col), ptr(self.val), 0, n, ptr(cnt), ptr(tmp_row),
              ptr(tmp_val), ptr(self.csc_ptr), ptr(self.csc_row), ptr(self.csc_val))

    def _edges(self, eps, window, cnt, row_ptr, col, val):
        _call('grl_jaccard_edges', ptr(self.row_ptr), ptr(self.col), ptr(self.val), ptr(self.csc_ptr),
              ptr(self.csc_row), ptr(self.csc_val), self.n, C.c_float(eps), window, ptr(cnt), ptr(row_ptr), ptr(col),
              ptr(val))

    def graph(self, eps, max_edges=None, return_dist=False, window=0):
        """``jaccard_graph``'s result for this state: count pass, grl_rrs_scan, one read-back of E, fill pass.
        ``window`` is grl_jaccard_edges' (0 = the library's; the result does not depend on it)."""
        n, dev = self.n, self.row_ptr.device
        limit = CLUSTER_MAX_EDGES if max_edges is None else int(max_edges)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        row_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self._edges(eps, window, cnt, None, None, None)
        _call('grl_rrs_scan', ptr(cnt), n, ptr(row_ptr))
        n_edges = int(row_ptr[n])
        if n_edges > limit:
            raise ValueError('jaccard_graph: eps = %r gives E = %d edges among %d samples, more than the limit of %d '
                             '(max_edges / GRL_CLUSTER_MAX_EDGES): lower eps or raise the limit'
                             % (eps, n_edges, n, limit))
        col = torch.empty(n_edges, dtype=torch.int32, device=dev)
        val = torch.empty(n_edges, dtype=torch.float32, device=dev) if return_dist else None
        if n_edges:
            self._edges(eps, window, None, row_ptr, col, val)
        return (row_ptr, col, val) if return_dist else (row_ptr, col)


def jaccard_graph(xf, eps, k1=20, k2=6, block_cols=None, block_bytes=None, max_edges=None, return_dist=False):
    """The eps-graph of the rows of ``xf`` [n, d] under the k-reciprocal Jaccard distance (the ``compute_jaccard_distance``
    of cluster-based re-ID, here the pure Jaccard term of ``re_ranking`` on the one-set Euclidean matrix)
    as a CSR ``(row_ptr int64 [n+1], col int32 [E])`` on the device, with ``return_dist`` also ``val`` float32 [E], the
    distance of every edge.  Edge i -> j (j != i) iff J[i][j] = 1 - t / (2 - t) <= float32(eps), t = the sum over the
    non-zero k of V2[i], ascending, of min(V2[i][k], V2[j][k]).  J lies in [0, 1]; 1 = no shared neighbour, so eps must
    be finite and < 1, and only pairs whose V2 rows overlap are ever looked at: no n x n pass after the two passes over
    the distance GEMM's column blocks that build V2.  Columns ascend in every row; the same bits on every run, for
    every ``block_cols`` / ``block_bytes``.  2 <= n, k1 <= 20, k1 < n, k2 <= 8, k2 <= n; any d >= 1 (rows are zero-padded
    to the multiple of 32 features the distance GEMM takes).  ValueError, before any device
    work: a host or non-2-d ``xf``, n < 2, k1 / k2 out of range, eps not finite or >= 1; after the count pass: E above
    ``max_edges`` (default GRL_CLUSTER_MAX_EDGES), before ``col`` is allocated.  Not sharded: under torch.distributed
    every rank computes the full, identical graph."""
    n, eps, k1, k2 = _jaccard_args(xf, eps, k1, k2, 'jaccard_graph')
    return _JaccardSet(xf, k1, k2, block_cols, block_bytes).graph(eps, max_edges, return_dist)


def cluster_jaccard(xf, eps, min_samples=1, k1=20, k2=6, block_cols=None, block_bytes=None, max_edges=None):
    """DBSCAN of the rows of ``xf`` on the k-reciprocal Jaccard distance at the threshold ``eps`` (0 <= J <= 1; 0.5 -
    0.6 in the clustering literature): ``cluster_from_graph(*jaccard_graph(xf, eps, k1, k2, ...), n, min_samples)``,
    the ``Clustering`` that ``cluster`` returns (``pair_scores``, ``centroids``).  A neighbourhood measured in shared
    k-reciprocal neighbours adapts to each identity's density, where one cosine threshold cannot.  Not sharded."""
    min_samples = _cluster_min_samples(min_samples, 'cluster_jaccard')
    n, eps, k1, k2 = _jaccard_args(xf, eps, k1, k2, 'cluster_jaccard')
    row_ptr, col = _JaccardSet(xf, k1, k2, block_cols, block_bytes).graph(eps, max_edges)
    return cluster_from_graph(row_ptr, col, n, min_samples, eps=eps, _checked=True)


# ----------------------------------------------------------------------------
# silhouette coefficients of a clustering over the distance GEMM's column blocks (silhouette.hip)
# ----------------------------------------------------------------------------
class Silhouette(object):
    """The result of ``silhouette`` / ``silhouette_matrix``:

      samples      float32 device [n]: s(i) = (b - a) / max(a, b); 0 for a sample whose cluster has one member
      a, b         float32 device [n]: the mean distance to the sample's own cluster (itself left out) and the smallest
                   mean distance to another cluster
      scored       bool device [n]: False for the samples ``noise='drop'`` left out (their samples / a / b are 0)
      score        float64: the mean of ``samples`` over the scored rows, NaN if one of them is NaN
      n_scored, n_clusters (the non-empty clusters, singletons included), metric, noise"""

    def __init__(self, samples, a, b, scored, score, n_scored, n_clusters, metric, noise):
        self.samples, self.a, self.b, self.scored = samples, a, b, scored
        self.score, self.n_scored, self.n_clusters, self.metric, self.noise = score, n_scored, n_clusters, metric, noise


def _silhouette_args(labels, n, noise, what):
    """The checks that need no device."""
    if noise not in ('singleton', 'drop'):
        raise ValueError("%s: noise must be 'singleton' or 'drop' (got %r)" % (what, noise))
    if not (torch.is_tensor(labels) and labels.dim() == 1 and labels.numel() == n
            and not labels.dtype.is_floating_point and not labels.dtype.is_complex and labels.dtype != torch.bool):
        raise ValueError('%s: labels must be an integer device tensor with one entry per sample (%d)' % (what, n))


def _silhouette_labels(labels, n, noise, what):
    """The clusters as the kernels take them: (labels int32 [n] with -1 = nobody's, counts int32 [k], mptr int64 [k+1],
    mem int32 [m], k, m, n_clusters).  Two read-backs: (max label, labels < 0) and the number of non-empty clusters."""
    if not labels.is_cuda:
        raise _lib.GrlHipError('labels must live on a HIP device (got %s): grl_amd has no CPU path' % labels.device)
    dev = labels.device
    lab = labels.to(torch.int64).clamp(min=-1)
    neg = lab < 0
    top, n_neg = (torch.stack((lab.max(), neg.sum())).tolist()) if n else (-1, 0)
    k = top + 1
    if noise == 'singleton' and n_neg:          # pair_scores' convention: every label < 0 is a cluster of its own
        lab = torch.where(neg, k - 1 + torch.cumsum(neg.to(torch.int64), 0), lab)
        k += n_neg
    if k > 2 ** 31 - 1:
        raise ValueError('%s: cluster ids must stay below 2^31 (got %d)' % (what, k - 1))
    if k < 2:
        raise ValueError('%s: the scored samples lie in fewer than 2 clusters' % what)
    lab32 = lab.to(torch.int32)
    counts = torch.zeros(k, dtype=torch.int32, device=dev)
    _call('grl_kmeans_label_counts', ptr(lab32), n, k, ptr(counts))
    n_clusters = int((counts > 0).sum())
    if n_clusters < 2:
        raise ValueError('%s: the scored samples lie in fewer than 2 clusters (%d)' % (what, n_clusters))
    mptr = torch.empty(k + 1, dtype=torch.int64, device=dev)
    _call('grl_rrs_scan', ptr(counts), k, ptr(mptr))
    cursor = torch.zeros(k, dtype=torch.int32, device=dev)
    tmp = torch.empty(n, dtype=torch.int32, device=dev)
    mem = torch.empty(n, dtype=torch.int32, device=dev)
    _call('grl_kmeans_members', ptr(lab32), n, k, ptr(mptr), ptr(cursor), ptr(tmp), ptr(mem))
    m = n - (n_neg if noise == 'drop' else 0)
    return lab32, counts, mptr, mem[:m], k, m, n_clusters


def _silhouette_width(n, m, block_cols, block_bytes):
    return _block_spans(n, 0, m, block_cols, block_bytes)[0]


def _silhouette_pass(block, n, width, cl, rinv, metric, noise):
    """The pass over the member order: ``block(c0, c1)`` -> the [n, c1 - c0] distances of every sample against the
    samples mem[c0:c1]; the blocks go to grl_silhouette_block in ascending position order on the current stream."""
    import numpy as np
    lab32, counts, mptr, mem, k, m, n_clusters = cl
    dev = lab32.device
    part = torch.empty((n, 64), dtype=torch.float32, device=dev)
    a = torch.empty(n, dtype=torch.float32, device=dev)
    b = torch.empty(n, dtype=torch.float32, device=dev)
    s = torch.empty(n, dtype=torch.float32, device=dev)
    rinv_pos = rinv[mem.to(torch.int64)] if rinv is not None else None
    for c0 in range(0, m, width):
        c1 = min(c0 + width, m)
        d = block(c0, c1)
        _call('grl_silhouette_block', ptr(d), d.stride(0), n, 0, c0, c1 - c0, ptr(mem), ptr(mptr), k, ptr(lab32),
              ptr(rinv), ptr(rinv_pos), ptr(part), ptr(a), ptr(b))
    _call('grl_silhouette_finish', ptr(a), ptr(b), ptr(lab32), ptr(counts), n, k, ptr(s))
    scored = lab32 >= 0
    host = s.cpu().numpy().astype(np.float64)[scored.cpu().numpy()]
    return Silhouette(s, a, b, scored, float(host.mean()), int(host.size), n_clusters, metric, noise)


def silhouette(xf, labels, metric='cosine', noise='singleton', block_cols=None, block_bytes=None):
    """The silhouette coefficient s(i) = (b - a) / max(a, b) of every row of ``xf`` [n, d] under ``labels`` (any integer
    device tensor [n]) as a ``Silhouette``: the label-free measure of a clustering, for choosing ``eps``,
    ``min_samples`` or ``k`` without ground truth.  a = the mean distance to the other members of the sample's cluster,
    b = the smallest mean distance to the members of another cluster; a cluster of one scores 0 (scikit-learn's rule).
    'cosine' is 1 - cos of the rows, which need not be unit: dist = max(0, 1 + (D * rinv_i) * rinv_j) with D =
    ``cosin_dist(xf, xf)`` and rinv = 1 / sqrt(grl_row_sqnorm) -- no normalised copy of ``xf`` is made; 'euclidean' is
    ``pairwise_distance_tensor(xf, xf)``.  ``noise``: 'singleton' (the convention of ``pair_scores``: every label < 0 is
    a cluster of its own and scores 0) or 'drop' (those samples are neither rows nor columns: ``samples`` 0, ``scored``
    False).  The distances come in column blocks of the MEMBER ORDER (the samples of cluster 0 ascending, then cluster
    1's, ..): the rows xf[mem[c0:c1]] are gathered into a buffer of the block's width and go through ``_ColumnBlocks``'
    GEMM, so every entry carries the full matrix's bits, and a small kernel folds the block into O(n) state.  No n x n,
    n x k or second n x d tensor exists (rows whose width is no multiple of 32 are zero-padded first, as the distance
    GEMM requires).  Every sum has a fixed order: the same bits on every run and for every block width.
    Cluster ids are used as they are (ids without members are skipped; the state holds max(label) + 1 counters).  Not
    sharded: under torch.distributed every rank computes the full, identical result.  ValueError: a ``verify_metric``,
    an unknown ``metric`` or ``noise``, labels that are not n integers, fewer than 2 non-empty clusters among the
    scored samples, ``xf`` without columns."""
    _cluster_metric(metric, 'silhouette')
    if not torch.is_tensor(xf) or xf.dim() < 2:
        raise ValueError('silhouette: xf must be a tensor [n, d] (got %s)'
                         % (tuple(xf.shape) if torch.is_tensor(xf) else type(xf).__name__,))
    _silhouette_args(labels, xf.shape[0], noise, 'silhouette')
    xf = _kmeans_rows(xf, 'silhouette')
    n = xf.shape[0]
    cl = _silhouette_labels(labels, n, noise, 'silhouette')
    mem, m = cl[3], cl[5]
    xf = _pad_features(xf)
    d = xf.shape[1]
    width = _silhouette_width(n, m, block_cols, block_bytes)
    rows = _new((width, d), xf)
    buf = _new((n * width,), xf)
    sq = _new((n,), xf)
    _call('grl_row_sqnorm', ptr(xf), ptr(sq), n, d, d)
    rinv = cn = None
    if metric == 'cosine':
        rinv = _new((n,), xf)
        _call('grl_silhouette_rinv', ptr(sq), n, ptr(rinv))
    else:
        cn = _new((width,), xf)
    mem64 = mem.to(torch.int64)

    def block(c0, c1):
        w = c1 - c0
        torch.index_select(xf, 0, mem64[c0:c1], out=rows[:w])
        out = buf[:n * w].view(n, w)
        if metric == 'cosine':
            return gemm(xf, rows[:w], out, n, w, d, epilogue=EPI_NEGDOT, math=MATH_F32)
        torch.index_select(sq, 0, mem64[c0:c1], out=cn[:w])
        return gemm(xf, rows[:w], out, n, w, d, epilogue=EPI_EUCLID, rnorm=sq, cnorm=cn[:w], math=MATH_F32)
    return _silhouette_pass(block, n, width, cl, rinv, metric, noise)


def silhouette_matrix(distmat, labels, noise='singleton', block_cols=None, block_bytes=None):
    """``silhouette`` on an [n, n] float32 distance matrix that already lives on the device, used as given (entry [i][j]
    is the distance of sample i to sample j; it need not be symmetric); rows may be strided.  The columns are gathered
    into the member order one block at a time.  ``metric`` of the result is 'precomputed'.  ValueError: not square."""
    if not torch.is_tensor(distmat) or distmat.dim() != 2 or distmat.shape[0] != distmat.shape[1]:
        raise ValueError('silhouette_matrix: distmat must be square [n, n] (got %s)'
                         % (tuple(distmat.shape) if torch.is_tensor(distmat) else type(distmat).__name__,))
    n = distmat.shape[0]
    _silhouette_args(labels, n, noise, 'silhouette_matrix')
    if distmat.dtype != torch.float32:
        raise ValueError('silhouette_matrix: distmat must be float32 (got %s)' % distmat.dtype)
    require_device(distmat, 'distmat')
    cl = _silhouette_labels(labels, n, noise, 'silhouette_matrix')
    mem, m = cl[3], cl[5]
    width = _silhouette_width(n, m, block_cols, block_bytes)
    buf = _new((n * width,), distmat)
    mem64 = mem.to(torch.int64)

    def block(c0, c1):
        out = buf[:n * (c1 - c0)].view(n, c1 - c0)
        return torch.index_select(distmat, 1, mem64[c0:c1], out=out)
    return _silhouette_pass(block, n, width, cl, None, 'precomputed', noise)


def cluster_select(xf, eps_list, min_samples=1, metric='cosine', score_metric=None, block_cols=None, block_bytes=None,
                   max_edges=None):
    """``cluster(xf, eps, min_samples, metric)`` at every eps of ``eps_list``, each result scored by
    ``silhouette(xf, labels, score_metric or metric, noise='singleton')`` -- noise as singletons, which score 0, so that
    shedding samples as noise cannot raise the score.  Returns ``(best Clustering, rows)``; ``rows`` is a list of dicts
    ``eps`` (the float32 compared with), ``n_clusters``, ``n_noise``, ``score`` in the order given, ``score`` None where
    fewer than 2 clusters exist.  The best is the highest finite score; ties go to the smaller eps.  ValueError: an
    empty list, no eps with a finite score."""
    import math
    score_metric = metric if score_metric is None else score_metric
    _cluster_metric(metric, 'cluster_select')
    _cluster_metric(score_metric, 'cluster_select')
    eps_list = [_cluster_eps(e, 'cluster_select') for e in eps_list]
    if not eps_list:
        raise ValueError('cluster_select: eps_list is empty')
    best, rows = None, []
    for eps in eps_list:
        cl = cluster(xf, eps, min_samples, metric, block_cols, block_bytes, max_edges)
        score = None
        if cl.n_clusters + cl.n_noise >= 2:
            score = silhouette(xf, cl.labels, score_metric, 'singleton', block_cols, block_bytes).score
        rows.append({'eps': eps, 'n_clusters': cl.n_clusters, 'n_noise': cl.n_noise, 'score': score})
        if score is not None and math.isfinite(score):
            if best is None or score > best[0] or (score == best[0] and eps < best[1]):
                best = (score, eps, cl)
    if best is None:
        raise ValueError('cluster_select: no eps of %r gives 2 or more clusters with a finite score' % (eps_list,))
    return best[2], rows


# ----------------------------------------------------------------------------
# HDBSCAN: the mutual-reachability minimum spanning forest over the distance GEMM's column blocks and the tree cut on
# its n - 1 edges (hdbscan.hip)
# ----------------------------------------------------------------------------
HDBSCAN_LAMBDA_FLOOR = 2.0 ** -126         # lambda = 1 / max(w, floor): an edge of weight 0 has a finite lambda
HDBSCAN_METHODS = ('eom', 'leaf')


class Hdbscan(object):
    """The result of ``hdbscan`` / ``hdbscan_matrix`` / ``hdbscan_from_mst``:

      labels       int64 device [n]: cluster id 0, 1, .. in ascending order of each cluster's smallest sample index; -1 = noise
      n_clusters, n_noise
      core_dist    float32 device [n]: the core distances (None from ``hdbscan_from_mst``)
      mst          (lo int32, hi int32, w float32) device [E]: the forest's edges, lo < hi, sorted by (w, lo, hi)
      stabilities  float64 numpy [n_clusters]: the stability of every selected cluster, in label order
      rounds       Boruvka rounds (passes over the distance blocks) the forest took; n_dropped: candidate edges dropped
                   because they would have closed a cycle (0 for a symmetric distance); both None from ``hdbscan_from_mst``
      min_cluster_size, min_samples, metric, method: the arguments of the call
      pair_scores(pids), centroids(xf, reduce='unit'), silhouette(xf, metric=None, noise='singleton'): as ``Clustering``'s"""

    def __init__(self, labels, n_clusters, n_noise, core_dist, mst, stabilities, rounds, n_dropped, min_cluster_size,
                 min_samples, metric, method):
        self.labels, self.n_clusters, self.n_noise = labels, n_clusters, n_noise
        self.core_dist, self.mst, self.stabilities = core_dist, mst, stabilities
        self.rounds, self.n_dropped = rounds, n_dropped
        self.min_cluster_size, self.min_samples, self.metric, self.method = min_cluster_size, min_samples, metric, method

    def pair_scores(self, pids):
        """``Clustering.pair_scores``: a noise point is a cluster of its own."""
        return _pair_scores(self.labels, self.n_clusters, pids)

    def centroids(self, xf, reduce='unit'):
        """``cluster_centroids(xf, labels, n_clusters, reduce)`` of the rows the labels were computed from."""
        return cluster_centroids(xf, self.labels, self.n_clusters, reduce)

    def silhouette(self, xf, metric=None, noise='singleton'):
        """``silhouette(xf, labels, metric, noise)``; ``metric`` defaults to the feature metric of the call ('cosine'
        for a result that has none)."""
        if metric is None:
            metric = self.metric if self.metric in ('cosine', 'euclidean') else 'cosine'
        return silhouette(xf, self.labels, metric, noise)


def _hdbscan_method(method, what):
    if method not in HDBSCAN_METHODS:
        raise ValueError("%s: method must be 'eom' or 'leaf' (got %r)" % (what, method))


def _hdbscan_args(min_cluster_size, min_samples, method, what):
    """(min_cluster_size, min_samples) as ints: the checks that need neither the device nor n."""
    mcs = _int_arg(min_cluster_size, 2, _INT_MAX, what, 'min_cluster_size')
    ms = mcs if min_samples is None else min_samples
    if min_samples is None and ms > SEARCH_K_MAX:
        raise ValueError('%s: min_samples defaults to min_cluster_size = %d, beyond %d; give min_samples' %
                         (what, ms, SEARCH_K_MAX))
    ms = _int_arg(ms, 1, SEARCH_K_MAX, what, 'min_samples')
    _hdbscan_method(method, what)
    return mcs, ms


def _hdbscan_min_samples_n(ms, n, what):
    if n >= 2 and ms > n:
        raise ValueError('%s: min_samples must be an integer in 1..min(n, %d) = %d (got %r)'
                         % (what, SEARCH_K_MAX, min(n, SEARCH_K_MAX), ms))


def _hdbscan_core_dist(blocks, n, min_samples, rinv):
    """The core distances float32 device [n]: one pass over the blocks into ``search``'s running top-min_samples lists
    (the cosine form applied to a block in place before it is ranked), the sample itself taken out."""
    dev = blocks.qf.device
    if min_samples == 1:
        return torch.zeros(n, dtype=torch.float32, device=dev)
    k = min_samples
    top = _TopK(n, k, dev)
    for c0, c1 in blocks.spans:
        d = blocks.block(c0, c1)
        if rinv is not None:
            _call('grl_hdbscan_cosine_block', ptr(d), d.stride(0), n, n, 0, c0, c1 - c0, ptr(rinv))
        top.push(d, d.stride(0), c1 - c0, c0)
    idx = top.key & 0xffffffff
    own = (idx == torch.arange(n, device=dev).unsqueeze(1)) & (torch.arange(k, device=dev) < k - 1).unsqueeze(0)
    # the sample is in its list before the last place: the last entry stays; otherwise the last one goes
    return torch.where(own.any(1), top.val[:, k - 1], top.val[:, k - 2]).contiguous()


def _mst_blocks(blocks, n, min_samples, rinv):
    """``mutual_reachability_mst`` over any block source (``_BlockSource``) of the n x n distance matrix;
    ``rinv``: the factors of the cosine form when the blocks hold -dot."""
    import numpy as np
    dev = blocks.qf.device
    prinv = ptr(rinv) if rinv is not None else None
    core = _hdbscan_core_dist(blocks, n, min_samples, rinv)
    # Boruvka rounds: one pass per round folds the blocks into each row's lightest outgoing edge; the per-component
    # minimum, the union-find and the new component ids run on the host over 2n read-back words
    comp = np.arange(n, dtype=np.int32)
    comp_d = torch.from_numpy(comp).to(dev)
    best_w = torch.empty(n, dtype=torch.float32, device=dev)
    best_j = torch.empty(n, dtype=torch.int32, device=dev)
    live = np.isfinite(core.cpu().numpy())
    parent = list(range(n))                                  # union-find over the samples (a list: scalar access)

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root
    cap = max(n - 1, 1).bit_length() + 1                     # ceil(log2 n) + 1
    e_lo, e_hi, e_w = [], [], []
    rounds = n_dropped = n_edges = 0
    n_live = int(live.sum())
    while n_live - n_edges > 1:                              # more than one component among the samples with a core distance
        if rounds >= cap:
            raise RuntimeError('mutual_reachability_mst: the forest did not settle in %d rounds' % cap)
        rounds += 1
        for c0, c1 in blocks.spans:
            d = blocks.block(c0, c1)
            _call('grl_hdbscan_minedge_block', ptr(d), d.stride(0), n, n, 0, c0, c1 - c0, ptr(core), ptr(comp_d), prinv,
                  ptr(best_w), ptr(best_j))
        bw, bj = best_w.cpu().numpy(), best_j.cpu().numpy().astype(np.int64)
        rows = np.flatnonzero(bj >= 0)
        if rows.size == 0:
            break
        lo, hi, w, c = np.minimum(rows, bj[rows]), np.maximum(rows, bj[rows]), bw[rows], comp[rows]
        order = np.lexsort((hi, lo, w, c))                   # by component, then the edges' total order
        cs = c[order]
        pick = order[np.concatenate(([True], cs[1:] != cs[:-1]))]       # every component's lightest outgoing edge
        pick = pick[np.lexsort((hi[pick], lo[pick], w[pick]))]
        plo, phi = lo[pick], hi[pick]
        twice = np.concatenate(([False], (plo[1:] == plo[:-1]) & (phi[1:] == phi[:-1])))     # both ends' components chose it
        pick, plo, phi = pick[~twice], plo[~twice], phi[~twice]
        took = []
        for k, (a, b) in enumerate(zip(plo.tolist(), phi.tolist())):
            ra, rb = find(a), find(b)
            if ra == rb:
                n_dropped += 1
                continue
            parent[max(ra, rb)] = min(ra, rb)
            took.append(k)
        e_lo.append(plo[took]); e_hi.append(phi[took]); e_w.append(w[pick][took])
        n_edges += len(took)
        up = np.asarray(parent, dtype=np.int64)
        while True:                                          # every sample's root: pointer jumping
            nxt = up[up]
            if np.array_equal(nxt, up):
                break
            up = nxt
        comp = up.astype(np.int32)
        comp_d = torch.from_numpy(comp).to(dev)
    lo = np.concatenate(e_lo).astype(np.int32) if e_lo else np.empty(0, dtype=np.int32)
    hi = np.concatenate(e_hi).astype(np.int32) if e_hi else np.empty(0, dtype=np.int32)
    w = np.concatenate(e_w).astype(np.float32) if e_w else np.empty(0, dtype=np.float32)
    order = np.lexsort((hi, lo, w))
    out = tuple(torch.from_numpy(np.ascontiguousarray(a[order])).to(dev) for a in (lo, hi, w))
    return out + (core, {'rounds': rounds, 'n_dropped': n_dropped})


def _mst_empty(n, dev):
    return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
            torch.empty(0, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
            {'rounds': 0, 'n_dropped': 0})


def mutual_reachability_mst(xf, min_samples, metric='cosine', block_cols=None, block_bytes=None):
    """The minimum spanning forest of the mutual-reachability graph of the rows of ``xf`` [n, d], without the n x n
    matrix: ``(lo int32 [E], hi int32 [E], w float32 [E], core float32 [n], info)`` on the device, lo < hi, the edges
    sorted by (w, lo, hi); ``info`` = {'rounds', 'n_dropped'}.  Distance of a pair {lo < hi}: 'euclidean' = the
    ``pairwise_distance_tensor(xf, xf)`` entry; 'cosine' = 1 - cos of the rows, which need not be unit, as
    max(0, 1 + (D * rinv[lo]) * rinv[hi]) with D = ``cosin_dist(xf, xf)`` and rinv = 1 / sqrt(grl_row_sqnorm), the
    smaller index first, so that both rows of a pair see the same bits.  core[i] = the distance to the
    (min_samples - 1)-th nearest other sample (the sample counts as its own neighbour at distance 0: scikit-learn's
    convention): row i of ``search``'s top-min_samples list with the entry of index i deleted, or the last entry if it
    is not there; +0 for min_samples = 1.  Edge weight w = max(dist, core[lo], core[hi]); a sample whose core distance
    is not finite has no edges, a w that is NaN or +inf is no edge.  Under the strict total order (w, lo, hi) the forest
    is unique.  It is built by Boruvka rounds: one pass over ``_ColumnBlocks``' distance blocks per round, each folded
    by grl_hdbscan_minedge_block into every row's lightest edge out of its component; the per-component minimum and
    the union-find run on the host over the 2n read-back words, n component ids go back.  At most ceil(log2 n) + 1
    rounds (RuntimeError beyond).  The same bits on every run and for every block width.  Not sharded: under
    torch.distributed every rank computes the full, identical result.  ValueError: a ``verify_metric``, an unknown
    metric, ``min_samples`` outside 1..min(n, 1024) or not an integer."""
    _cluster_metric(metric, 'mutual_reachability_mst')
    min_samples = _int_arg(min_samples, 1, SEARCH_K_MAX, 'mutual_reachability_mst', 'min_samples')
    if not torch.is_tensor(xf) or xf.dim() < 2:
        raise ValueError('mutual_reachability_mst: xf must be a tensor [n, d] (got %s)'
                         % (tuple(xf.shape) if torch.is_tensor(xf) else type(xf).__name__,))
    n = xf.shape[0]
    _hdbscan_min_samples_n(min_samples, n, 'mutual_reachability_mst')
    require_device(xf, 'xf')
    if n <= 1:                             # (nothing to launch)
        return _mst_empty(n, xf.device)
    xf = _pad_features(_kmeans_rows(xf, 'mutual_reachability_mst'))
    blocks = _ColumnBlocks(xf, xf, metric, block_cols, block_bytes)
    rinv = None
    if metric == 'cosine':
        d = xf.shape[1]
        sq, rinv = _new((n,), xf), _new((n,), xf)
        _call('grl_row_sqnorm', ptr(xf), ptr(sq), n, d, d)
        _call('grl_silhouette_rinv', ptr(sq), n, ptr(rinv))
    return _mst_blocks(blocks, n, min_samples, rinv)


def _hdbscan_cut(lo, hi, w, n, mcs, method):
    """The cut of DESIGN.md 4x on the host in float64: (labels int64 [n], n_clusters, stabilities float64 [n_clusters])
    from the forest's edges in their sorted order."""
    import numpy as np
    m = len(lo)
    uf = list(range(n))

    def find(a):
        root = a
        while uf[root] != root:
            root = uf[root]
        while uf[a] != root:
            uf[a], a = root, uf[a]
        return root
    # single-linkage dendrogram: merge k is node n + k, its children the two current tops
    top = list(range(n))
    left, right = [0] * m, [0] * m
    size = [1] * n + [0] * m
    for k in range(m):
        a, b = find(lo[k]), find(hi[k])
        if a == b:
            raise ValueError('hdbscan_from_mst: the edges are not a forest (edge %d closes a cycle)' % k)
        left[k], right[k] = top[a], top[b]
        size[n + k] = size[top[a]] + size[top[b]]
        r = min(a, b)
        uf[max(a, b)] = r
        top[r] = n + k
    big = [top[r] for r in range(n) if uf[r] == r and size[top[r]] >= mcs]
    # condensed tree, top-down; cluster ids are handed out parents first
    birth, stab, cparent, kids, selectable = [], [], [], [], []

    def new_cluster(lam, par, sel):
        birth.append(lam); stab.append(0.0); cparent.append(par); kids.append([]); selectable.append(sel)
        return len(birth) - 1
    left_in = np.full(n, -1, dtype=np.int64)                # the cluster every point left

    def leave(node, c):
        todo = [node]
        while todo:
            v = todo.pop()
            if v < n:
                left_in[v] = c
            else:
                todo.append(left[v - n]); todo.append(right[v - n])
    stack = [(t, new_cluster(0.0, -1, len(big) >= 2)) for t in big]
    while stack:
        node, c = stack.pop()
        while node >= n:
            k = node - n
            lam = 1.0 / max(float(w[k]), HDBSCAN_LAMBDA_FLOOR)
            a, b = left[k], right[k]
            sa, sb = size[a], size[b]
            if sa >= mcs and sb >= mcs:                      # a true split: two clusters are born
                stab[c] += (sa + sb) * (lam - birth[c])
                for ch in (a, b):
                    cid = new_cluster(lam, c, True)
                    kids[c].append(cid)
                    stack.append((ch, cid))
                break
            if sa >= mcs or sb >= mcs:                       # the cluster goes on, the small side's points leave
                small, node = (b, a) if sa >= mcs else (a, b)
                stab[c] += size[small] * (lam - birth[c])
                leave(small, c)
                continue
            stab[c] += (sa + sb) * (lam - birth[c])          # the cluster dissolves
            leave(node, c)
            break
    ncl = len(birth)
    chosen = [False] * ncl
    if method == 'leaf':
        chosen = [selectable[c] and not kids[c] for c in range(ncl)]
    else:
        value = list(stab)
        for c in range(ncl - 1, -1, -1):
            if not kids[c]:
                chosen[c] = selectable[c]
                continue
            tot = value[kids[c][0]] + value[kids[c][1]]
            if not selectable[c] or tot > stab[c]:
                value[c] = tot
            else:
                chosen[c] = True
    at = [-1] * ncl                                          # the selected cluster at or above c
    for c in range(ncl):
        up = at[cparent[c]] if cparent[c] >= 0 else -1
        at[c] = up if up >= 0 else (c if chosen[c] else -1)
    at = np.asarray(at + [-1], dtype=np.int64)               # (left_in == -1 reads the appended -1)
    raw = at[left_in]
    labels = np.full(n, -1, dtype=np.int64)
    keep = raw >= 0
    ids, first = np.unique(raw[keep], return_index=True)     # first = each cluster's smallest sample index (in keep)
    rank = np.empty(ids.size, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(ids.size)
    labels[keep] = rank[np.searchsorted(ids, raw[keep])]
    stabilities = np.zeros(ids.size, dtype=np.float64)
    stabilities[rank] = np.asarray([stab[c] for c in ids.tolist()], dtype=np.float64)
    return labels, int(ids.size), stabilities


def _hdbscan_result(mst, core, info, n, mcs, ms, metric, method, dev):
    import numpy as np
    lo, hi, w = (t.cpu().numpy() for t in mst)
    labels, n_clusters, stabilities = _hdbscan_cut(lo.tolist(), hi.tolist(), w.astype(np.float64), n, mcs, method)
    return Hdbscan(torch.from_numpy(labels).to(dev), n_clusters, int((labels < 0).sum()), core, mst, stabilities,
                   info.get('rounds'), info.get('n_dropped'), mcs, ms, metric, method)


def hdbscan_from_mst(lo, hi, w, n, min_cluster_size, method='eom'):
    """HDBSCAN's labels from a mutual-reachability forest (``mutual_reachability_mst``'s device arrays lo int32, hi
    int32, w float32 [E]) as an ``Hdbscan``.  The forest depends on ``min_samples`` only, so another
    ``min_cluster_size`` or ``method`` costs no GPU pass.  The cut runs on the host in float64 over the E <= n - 1
    edges, in the edges' order (w, lo, hi): the single-linkage dendrogram by union-find; condensed top-down at lambda =
    1 / max(w, 2^-126) -- two children of at least ``min_cluster_size`` samples are two new clusters, one such child
    goes on as the same cluster while the other's points leave, none dissolves the cluster; stability = the sum over
    leaving points and child clusters of size * (lambda - lambda_birth); 'eom' selects bottom-up (children whose total
    exceeds the parent's own stability replace it), 'leaf' the leaves.  A forest of one component of at least
    ``min_cluster_size`` samples has that component as the never-selected root (scikit-learn's
    allow_single_cluster=False); with two or more, each is a selectable cluster born at lambda = 0; smaller components
    are noise.  ValueError: arrays that are not E edges with 0 <= lo < hi < n, edges that close a cycle,
    ``min_cluster_size`` < 2, an unknown method."""
    import numpy as np
    mcs = _int_arg(min_cluster_size, 2, _INT_MAX, 'hdbscan_from_mst', 'min_cluster_size')
    _hdbscan_method(method, 'hdbscan_from_mst')
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError('hdbscan_from_mst: n must be an integer >= 0 (got %r)' % (n,))
    n = int(n)
    for t, dt, what in ((lo, torch.int32, 'lo'), (hi, torch.int32, 'hi'), (w, torch.float32, 'w')):
        if not (torch.is_tensor(t) and t.dtype == dt and t.dim() == 1 and t.numel() == lo.numel()):
            raise ValueError('hdbscan_from_mst: %s must be a 1-d %s device tensor, one entry per edge' % (what, dt))
    if not (lo.is_cuda and hi.is_cuda and w.is_cuda):
        raise _lib.GrlHipError('lo, hi and w must live on a HIP device (got %s): grl_amd has no CPU path' % lo.device)
    a, b, ww = lo.cpu().numpy(), hi.cpu().numpy(), w.cpu().numpy()
    if a.size and not ((a >= 0) & (a < b) & (b < n)).all():
        raise ValueError('hdbscan_from_mst: every edge needs 0 <= lo < hi < n = %d' % n)
    if np.isnan(ww).any():
        raise ValueError('hdbscan_from_mst: a NaN weight is no edge')
    order = np.lexsort((b, a, ww))
    mst = tuple(t[torch.from_numpy(order).to(lo.device)] for t in (lo, hi, w))
    return _hdbscan_result(mst, None, {}, n, mcs, None, None, method, lo.device)


def hdbscan(xf, min_cluster_size=5, min_samples=None, metric='cosine', method='eom', block_cols=None, block_bytes=None):
    """HDBSCAN of the rows of ``xf`` [n, d] as an ``Hdbscan``: the density clustering that needs no ``eps`` and copes
    with identities of different spread.  ``hdbscan_from_mst(*mutual_reachability_mst(xf, min_samples, metric, ..),
    n, min_cluster_size, method)``; ``min_samples=None`` means ``min_cluster_size``.  No n x n matrix exists on the
    device or the host: 1 + rounds passes over the distance GEMM's column blocks (rounds <= ceil(log2 n) + 1), and the
    host sees the n - 1 edges and n labels.  On distances without ties among the mutual-reachability weights the
    partition is scikit-learn's HDBSCAN(metric='precomputed', allow_single_cluster=False); with ties the dendrogram
    follows the edges' order (w, lo, hi) where scikit-learn's follows its sort.  n = 0 and n = 1 give an
    empty / all-noise result without a launch.  Not sharded.  ValueError: a ``verify_metric``, an unknown metric or
    method, ``min_cluster_size`` < 2, ``min_samples`` outside 1..min(n, 1024), bool or non-integer arguments."""
    _cluster_metric(metric, 'hdbscan')
    mcs, ms = _hdbscan_args(min_cluster_size, min_samples, method, 'hdbscan')
    lo, hi, w, core, info = mutual_reachability_mst(xf, ms, metric, block_cols, block_bytes)
    return _hdbscan_result((lo, hi, w), core, info, xf.shape[0], mcs, ms, metric, method, lo.device)


def hdbscan_matrix(distmat, min_cluster_size=5, min_samples=None, method='eom', block_cols=None):
    """``hdbscan`` on an [n, n] float32 distance matrix that already lives on the device, the entries used as they are;
    rows may be strided (a column slice of a wider matrix is read in place), and ``block_cols`` cuts it into column
    slices that are read in place too.  The matrix must be symmetric bit for bit: a row pass sees only row i's view
    of a pair, and the two views have to agree on the edge.  ``metric`` of the result is 'precomputed'.  ValueError:
    not square, not float32, not symmetric, and ``hdbscan``'s."""
    mcs, ms = _hdbscan_args(min_cluster_size, min_samples, method, 'hdbscan_matrix')
    if not torch.is_tensor(distmat) or distmat.dim() != 2 or distmat.shape[0] != distmat.shape[1]:
        raise ValueError('hdbscan_matrix: distmat must be square [n, n] (got %s)'
                         % (tuple(distmat.shape) if torch.is_tensor(distmat) else type(distmat).__name__,))
    if distmat.dtype != torch.float32:
        raise ValueError('hdbscan_matrix: distmat must be float32 (got %s)' % distmat.dtype)
    n = distmat.shape[0]
    _hdbscan_min_samples_n(ms, n, 'hdbscan_matrix')
    require_device(distmat, 'distmat')
    dev = distmat.device
    if n <= 1:
        lo, hi, w, core, info = _mst_empty(n, dev)
        return _hdbscan_result((lo, hi, w), core, info, n, mcs, ms, 'precomputed', method, dev)
    if distmat.stride(1) != 1 or distmat.stride(0) < n:
        distmat = distmat.contiguous()
    bits = distmat.view(torch.int32)
    if not torch.equal(bits, bits.t()):
        raise ValueError('hdbscan_matrix: distmat must be symmetric bit for bit (a row pass sees one view of a pair)')
    width = n if block_cols is None else max(1, min(int(block_cols), n))

    class _Slices(object):                          # a block source of column slices of the matrix itself
        spans = [(c, min(c + width, n)) for c in range(0, n, width)]
        qf = distmat

        @staticmethod
        def block(c0, c1):
            return distmat[:, c0:c1]
    lo, hi, w, core, info = _mst_blocks(_Slices, n, ms, None)
    return _hdbscan_result((lo, hi, w), core, info, n, mcs, ms, 'precomputed', method, dev)


# ----------------------------------------------------------------------------
# t-SNE map of a feature set (tsne.hip)
# ----------------------------------------------------------------------------
TSNE_METRICS = ('cosine', 'euclidean')


class Tsne(object):
    """The result of ``tsne`` / ``tsne_from_affinities``:

      embedding      float32 device [n, 2]; the row of an isolated sample is NaN
      kl             the Kullback-Leibler divergence sum P log(P Z / q) over the stored affinities at ``embedding``
      n_iter         iterations run;  n_isolated: samples without affinities
      perplexity, metric, seed (None for a given ``init``), learning_rate (the float that was used)
      affinities     (row_ptr int64 [n + 1], col int32 [E], val float32 [E]): the joint affinities, a CSR on the device
      beta           float32 device [n]: every sample's precision (None from ``tsne_from_affinities``)
      isolated       bool device [n]
      gains, update  float32 device [n, 2]: the optimiser's state after the last iteration"""

    def __init__(self, embedding, kl, n_iter, n_isolated, perplexity, metric, seed, learning_rate, affinities, beta,
                 isolated, gains, update):
        self.embedding, self.kl, self.n_iter, self.n_isolated = embedding, kl, n_iter, n_isolated
        self.perplexity, self.metric, self.seed, self.learning_rate = perplexity, metric, seed, learning_rate
        self.affinities, self.beta, self.isolated, self.gains, self.update = affinities, beta, isolated, gains, update


def _tsne_real(v, what, name):
    import math
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError('%s: %s must be a finite number (got %r)' % (what, name, v))
    return float(v)


def _tsne_rows(xf, perplexity, metric, what):
    """The checks of ``tsne`` / ``tsne_affinities`` that need no device work: (n, K, perplexity as a float)."""
    if isinstance(metric, VerifyMetric):
        raise ValueError('%s: a verify_metric is the signed logit of modified query rows against gallery rows, not a '
                         "distance between two samples of one set; embed by 'cosine' or 'euclidean'" % what)
    if metric not in TSNE_METRICS:
        raise ValueError("%s: metric must be 'cosine' or 'euclidean' (got %r)" % (what, metric))
    if not (torch.is_tensor(xf) and xf.is_cuda and xf.dtype == torch.float32 and xf.dim() == 2):
        raise ValueError('%s: xf must be a 2-d float32 tensor [n, d] on a HIP device (got %s)'
                         % (what, '%s %s on %s' % (tuple(xf.shape), xf.dtype, xf.device) if torch.is_tensor(xf)
                            else type(xf).__name__))
    n = int(xf.shape[0])
    if n < 3 or xf.shape[1] < 1:
        raise ValueError('%s: needs n >= 3 samples of d >= 1 features (got %s)' % (what, tuple(xf.shape)))
    perp = _tsne_real(perplexity, what, 'perplexity')
    K = min(n - 1, int(3.0 * perp) + 1) if perp >= 1.0 else 0
    if K + 1 > SEARCH_K_MAX:
        raise ValueError('%s: perplexity = %r needs %d neighbours, search holds %d: perplexity must be below %d'
                         % (what, perplexity, K, SEARCH_K_MAX - 1, (SEARCH_K_MAX - 1) // 3))
    if not 1.0 <= perp < K:
        raise ValueError('%s: perplexity must be a number in [1, K) with K = min(n - 1, floor(3 perplexity) + 1) = %d '
                         'neighbours, or the target entropy cannot be reached (got %r for n = %d)' % (what, K, perplexity, n))
    return n, K, perp


def _tsne_optimiser(n_iter, learning_rate, early_exaggeration, exaggeration_iter, seed, init, n, what):
    """The optimiser arguments checked without device work: (n_iter, lr or None for 'auto', alpha, switch, seed)."""
    n_iter = _int_arg(n_iter, 1, None, what, 'n_iter')
    exaggeration_iter = _int_arg(exaggeration_iter, 0, None, what, 'exaggeration_iter')
    lr = None
    if not (isinstance(learning_rate, str) and learning_rate == 'auto'):
        lr = _tsne_real(learning_rate, what, 'learning_rate')
        if lr <= 0:
            raise ValueError("%s: learning_rate must be 'auto' or a number > 0 (got %r)" % (what, learning_rate))
    alpha = _tsne_real(early_exaggeration, what, 'early_exaggeration')
    if alpha <= 0:
        raise ValueError('%s: early_exaggeration must be > 0 (got %r)' % (what, early_exaggeration))
    if torch.is_tensor(init):
        if not (init.is_cuda and init.dtype == torch.float32 and tuple(init.shape) == (n, 2)):
            raise ValueError('%s: an init tensor must be float32 [n, 2] = [%d, 2] on a HIP device (got %s %s on %s)'
                             % (what, n, tuple(init.shape), init.dtype, init.device))
        seed = None
    elif isinstance(init, str) and init == 'random':
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError('%s: seed must be an integer >= 0 (got %r)' % (what, seed))
        seed = int(seed)
    else:
        raise ValueError("%s: init must be 'random' or a float32 [n, 2] device tensor (got %r)" % (what, init))
    return n_iter, lr, alpha, exaggeration_iter, seed


def _tsne_csr(row_ptr, col, val, isolated, what, checked=False):
    """A caller's CSR checked: the shapes and dtypes without device work, then (one read-back) that it is square and
    that the columns ascend in every row.  Returns (n, isolated as uint8 or None)."""
    for t, dt, name in ((row_ptr, torch.int64, 'row_ptr'), (col, torch.int32, 'col'), (val, torch.float32, 'val')):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 1):
            raise ValueError('%s: %s must be a 1-d %s tensor on a HIP device' % (what, name, dt))
    n = row_ptr.numel() - 1
    if n < 1 or col.numel() != val.numel():
        raise ValueError('%s: row_ptr must hold n + 1 >= 2 entries, col and val one entry per stored affinity' % what)
    if isolated is not None:
        if not (torch.is_tensor(isolated) and isolated.is_cuda and isolated.dtype in (torch.bool, torch.uint8)
                and tuple(isolated.shape) == (n,)):
            raise ValueError('%s: isolated must be a bool [n] = [%d] tensor on a HIP device' % (what, n))
        isolated = isolated.to(torch.uint8).contiguous()
    if not checked:
        E = col.numel()
        lens = row_ptr[1:] - row_ptr[:-1]
        ok = (row_ptr[0] == 0) & (row_ptr[n] == E) & (lens >= 0).all()
        if E:
            ok = ok & (col >= 0).all() & (col < n).all()
        if not bool(ok):
            raise ValueError('%s: the CSR is not square: row_ptr must run from 0 to E = %d without a step down and every '
                             'column lie in 0..n-1 = 0..%d' % (what, E, n - 1))
        if E > 1:
            rows = torch.repeat_interleave(torch.arange(n, device=col.device), lens)
            if bool(((rows[1:] == rows[:-1]) & (col[1:] <= col[:-1])).any()):
                raise ValueError('%s: the CSR is not sorted: the columns of a row must ascend, each once' % what)
    return n, isolated


def tsne_affinities(xf, perplexity=30.0, metric='cosine', block_cols=None, block_bytes=None):
    """The joint affinities P of t-SNE for the rows of ``xf`` [n, d] as a CSR on the device, without the n x n matrix:
    ``(row_ptr int64 [n + 1], col int32 [E], val float32 [E], info)``.  Distance of a pair: 'cosine' = the symmetric
    chain of ``mutual_reachability_mst`` (for unit rows half the squared Euclidean distance, used as it is),
    'euclidean' = the square of the ``pairwise_distance_tensor(xf, xf)`` entry.  Every sample keeps its K =
    min(n - 1, floor(3 perplexity) + 1) nearest neighbours: row i of ``search``'s top-(K + 1) list with the entry of
    index i deleted, or the last entry if it is not there -- one pass over ``_ColumnBlocks``.  grl_tsne_perplexity then
    runs scikit-learn's bisection on every row's precision beta in fp32.  A sample whose list holds a distance that is
    not finite is isolated: it has no affinities in either direction.  P[i][j] = (p(j|i) + p(i|j)) / (2 n_live) over the
    union pattern, columns ascending, symmetric bit for bit; a row may hold up to n - 1 entries.  ``info``: idx int32
    [n, K], e and cond float32 [n, K], beta float32 [n], isolated bool [n], K.  The same bits on every run and for every
    block width.  Not sharded: under torch.distributed every rank computes the identical result, no collective.
    ValueError, before any device work: a host or non-2-d ``xf``, n < 3, a perplexity outside [1, K) or a bool, an
    unknown metric, a ``verify_metric``."""
    import math
    n, K, perp = _tsne_rows(xf, perplexity, metric, 'tsne_affinities')
    dev = xf.device
    xf = _pad_features(xf)
    blocks = _ColumnBlocks(xf, xf, metric, block_cols, block_bytes)
    rinv = None
    if metric == 'cosine':
        d = xf.shape[1]
        sq, rinv = _new((n,), xf), _new((n,), xf)
        _call('grl_row_sqnorm', ptr(xf), ptr(sq), n, d, d)
        _call('grl_silhouette_rinv', ptr(sq), n, ptr(rinv))
    top = _TopK(n, K + 1, dev)
    for c0, c1 in blocks.spans:
        d = blocks.block(c0, c1)
        if rinv is not None:
            _call('grl_hdbscan_cosine_block', ptr(d), d.stride(0), n, n, 0, c0, c1 - c0, ptr(rinv))
        else:
            _call('grl_tsne_square_block', ptr(d), d.stride(0), n, c1 - c0)
        top.push(d, d.stride(0), c1 - c0, c0)
    del blocks
    # the sample's own entry goes, or the last one when it is not in the list
    idx = top.key & 0xffffffff
    own = idx == torch.arange(n, device=dev).unsqueeze(1)
    drop = torch.where(own.any(1), own.to(torch.int32).argmax(1), torch.full((n,), K, dtype=torch.int64, device=dev))
    take = torch.arange(K, device=dev).unsqueeze(0)
    take = take + (take >= drop.unsqueeze(1)).to(torch.int64)
    e = top.val.gather(1, take).contiguous()
    idx = idx.gather(1, take).to(torch.int32).contiguous()
    del top
    cond = torch.empty((n, K), dtype=torch.float32, device=dev)
    beta = torch.empty(n, dtype=torch.float32, device=dev)
    iso = torch.empty(n, dtype=torch.uint8, device=dev)
    _call('grl_tsne_perplexity', ptr(e), n, K, float(math.log(perp)), ptr(cond), ptr(beta), ptr(iso))
    isolated = iso.bool()
    n_live = n - int(isolated.sum())
    info = {'idx': idx, 'e': e, 'cond': cond, 'beta': beta, 'isolated': isolated, 'K': K}
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n_live == 0:
        return (row_ptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                info)
    # the conditional matrix by rows (columns ascending, the pairs with an isolated end marked -1) and by columns
    acol = torch.where(isolated.unsqueeze(1) | isolated[idx.long()], torch.full_like(idx, -1), idx).contiguous()
    m = n * K
    flat_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * K
    csc_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    csc_row = torch.zeros(m, dtype=torch.int32, device=dev)
    csc_val = torch.zeros(m, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    tmp_row = torch.empty(m, dtype=torch.int32, device=dev)
    tmp_val = torch.empty(m, dtype=torch.float32, device=dev)
    _call('grl_rrs_transpose', ptr(flat_ptr), ptr(acol), ptr(cond), 0, n, ptr(cnt), ptr(tmp_row), ptr(tmp_val),
          ptr(csc_ptr), ptr(csc_row), ptr(csc_val))
    del tmp_row, tmp_val
    acol, order = torch.sort(acol, dim=1)                     # (a row's live columns are distinct: one order)
    acol = acol.contiguous()
    aval = cond.gather(1, order).contiguous()
    den = C.c_float(2.0 * n_live)

    def joint(rp, col, val):
        _call('grl_tsne_joint', ptr(acol), ptr(aval), K, ptr(csc_ptr), ptr(csc_row), ptr(csc_val), n, den, rp, ptr(cnt),
              col, val)
    joint(None, None, None)
    _call('grl_rrs_scan', ptr(cnt), n, ptr(row_ptr))
    n_entries = int(row_ptr[n])
    col = torch.empty(max(n_entries, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(n_entries, 1), dtype=torch.float32, device=dev)
    joint(ptr(row_ptr), ptr(col), ptr(val))
    return row_ptr, col[:n_entries], val[:n_entries], info


def _tsne_terms(y, iso, n, rep, rowz, z):
    """rep, rowz and Z at y: the two launches every gradient starts with."""
    _call('grl_tsne_repulsion', ptr(y), ptr(iso), n, ptr(rep), ptr(rowz))
    _call('grl_tsne_z', ptr(rowz), n, ptr(z))


def tsne_gradient(row_ptr, col, val, y, exaggeration=1.0, isolated=None):
    """The exact t-SNE gradient at ``y`` [n, 2] for the joint affinities of a CSR (``tsne_affinities``' or a caller's:
    row_ptr int64 [n + 1], col int32 ascending in every row, val float32): ``(grad float32 [n, 2], z float32 [1])`` on
    the device.  For a live i: dx = y[i] - y[j], q = 1 / (1 + |dx|^2); rep[i] = sum over the live j != i of q q dx,
    Z = sum over i of sum over j of q, att[i] = sum over the row's entries of (exaggeration P) q dx, grad[i] =
    4 (att[i] - rep[i] / Z).  The repulsive term is the exact n-body sum, computed on the fly; every sum runs in the
    fixed fp32 order of DESIGN.md 4y, so the result is the same bit for bit on every run.  ``isolated`` bool [n]: samples
    that exert no force and feel none (their gradient is 0).  ValueError: arrays of the wrong shape, dtype or device, a
    CSR that is not square or not sorted."""
    n, iso = _tsne_csr(row_ptr, col, val, isolated, 'tsne_gradient')
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (n, 2)):
        raise ValueError('tsne_gradient: y must be a float32 [n, 2] = [%d, 2] tensor on a HIP device' % n)
    alpha = _tsne_real(exaggeration, 'tsne_gradient', 'exaggeration')
    y = y.contiguous()
    dev = y.device
    rep, grad = torch.empty_like(y), torch.empty_like(y)
    rowz = torch.empty(n, dtype=torch.float32, device=dev)
    z = torch.empty(1, dtype=torch.float32, device=dev)
    _tsne_terms(y, iso, n, rep, rowz, z)
    _call('grl_tsne_update', ptr(row_ptr), ptr(col), ptr(val), ptr(y), ptr(iso), n, alpha, ptr(rep), ptr(z), ptr(grad),
          None, None, None, 0.0, 0.0)
    return grad, z


def _tsne_run(row_ptr, col, val, iso, n, n_iter, lr, alpha, switch, seed, init, first=0, gains=None, update=None):
    """The loop: three launches an iteration on the current stream, nothing read back inside it.  Returns
    (y, gains, update, kl)."""
    import numpy as np
    dev = row_ptr.device
    if seed is not None:
        y0 = np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 2)).astype(np.float32) * np.float32(1e-4)
        y = torch.from_numpy(y0).to(dev)
    else:
        y = init.contiguous().clone()
    y2, rep = torch.empty_like(y), torch.empty_like(y)
    gains = torch.ones_like(y) if gains is None else gains.contiguous().clone()
    update = torch.zeros_like(y) if update is None else update.contiguous().clone()
    rowz = torch.empty(n, dtype=torch.float32, device=dev)
    z = torch.empty(1, dtype=torch.float32, device=dev)
    args = (ptr(row_ptr), ptr(col), ptr(val))
    for it in range(first, first + n_iter):
        early = it < switch
        _tsne_terms(y, iso, n, rep, rowz, z)
        _call('grl_tsne_update', *args, ptr(y), ptr(iso), n, alpha if early else 1.0, ptr(rep), ptr(z), None,
              ptr(gains), ptr(update), ptr(y2), 0.5 if early else 0.8, lr)
        y, y2 = y2, y
    _tsne_terms(y, iso, n, rep, rowz, z)
    _call('grl_tsne_kl', *args, ptr(y), ptr(iso), n, ptr(z), ptr(rowz))
    kl = float(rowz.double().sum())
    return y, gains, update, kl


def _tsne_lr(lr, n_live, alpha):
    import numpy as np
    return float(np.float32(max(n_live / alpha / 4.0, 50.0) if lr is None else lr))


def tsne_from_affinities(row_ptr, col, val, n_iter=1000, seed=0, init='random', learning_rate='auto',
                         early_exaggeration=12.0, exaggeration_iter=250, isolated=None, first_iter=0, gains=None,
                         update=None):
    """The t-SNE loop on joint affinities that are there already (``tsne_affinities``' CSR or a caller's): a second seed
    or more iterations cost no distance pass.  The arguments are ``tsne``'s.  ``init`` = an earlier run's ``embedding``
    (with its NaN rows replaced), ``gains`` / ``update`` its state and ``first_iter`` the iterations it ran continue that
    run bit for bit.  Returns a ``Tsne`` (``perplexity``, ``metric`` and ``beta`` are None)."""
    what = 'tsne_from_affinities'
    n, iso = _tsne_csr(row_ptr, col, val, isolated, what, checked=True)            # (the checks without device work first)
    n_iter, lr, alpha, switch, seed = _tsne_optimiser(n_iter, learning_rate, early_exaggeration, exaggeration_iter, seed,
                                                      init, n, what)
    if isinstance(first_iter, bool) or not isinstance(first_iter, numbers.Integral) or first_iter < 0:
        raise ValueError('%s: first_iter must be an integer >= 0 (got %r)' % (what, first_iter))
    for t, name in ((gains, 'gains'), (update, 'update')):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
                                  and tuple(t.shape) == (n, 2)):
            raise ValueError('%s: %s must be a float32 [n, 2] = [%d, 2] tensor on a HIP device' % (what, name, n))
    _tsne_csr(row_ptr, col, val, isolated, what)
    return _tsne_result(row_ptr, col, val, iso, n, n_iter, lr, alpha, switch, seed, init, None, None, None, int(first_iter),
                        gains, update)


def _tsne_result(row_ptr, col, val, iso, n, n_iter, lr, alpha, switch, seed, init, perp, metric, beta, first=0,
                 gains=None, update=None):
    dev = row_ptr.device
    n_iso = int(iso.sum()) if iso is not None else 0
    lr = _tsne_lr(lr, n - n_iso, alpha)
    if n_iso == n:                                   # nobody has an affinity: nothing moves, nothing is launched
        y = torch.full((n, 2), float('nan'), dtype=torch.float32, device=dev)
        return Tsne(y, 0.0, n_iter, n_iso, perp, metric, seed, lr, (row_ptr, col, val), beta, iso.bool(),
                    torch.ones_like(y), torch.zeros_like(y))
    y, gains, update, kl = _tsne_run(row_ptr, col, val, iso, n, n_iter, lr, alpha, switch, seed, init, first, gains, update)
    isolated = iso.bool() if iso is not None else torch.zeros(n, dtype=torch.bool, device=dev)
    if n_iso:
        y[isolated] = float('nan')
    return Tsne(y, kl, n_iter, n_iso, perp, metric, seed, lr, (row_ptr, col, val), beta, isolated, gains, update)


def tsne(xf, perplexity=30.0, metric='cosine', n_iter=1000, seed=0, init='random', learning_rate='auto',
         early_exaggeration=12.0, exaggeration_iter=250, block_cols=None, block_bytes=None):
    """The 2-d t-SNE map of the rows of ``xf`` [n, d] on the device as a ``Tsne``: scikit-learn's exact gradient with
    the affinities restricted to every sample's nearest neighbours (``tsne_affinities``), no n x n matrix, no tree, no
    approximation.  ``init='random'`` draws Generator(PCG64(seed)).standard_normal((n, 2)) as float32 times 1e-4 on the
    host; a float32 [n, 2] device tensor is used as it is.  Exactly ``n_iter`` iterations of scikit-learn's update
    (gains + 0.2 / * 0.8 floored at 0.01, momentum 0.5 and the affinities times ``early_exaggeration`` for the first
    ``exaggeration_iter`` iterations, then 0.8 and 1): three launches each -- the exact repulsive n-body sum, Z, the
    sparse attraction with the update -- and no read-back inside the loop.  ``learning_rate='auto'`` = max(n_live /
    early_exaggeration / 4, 50).  The Kullback-Leibler divergence at the final map is reported and steers nothing: no
    early stopping.  The same bits on every run and for every block width.  Not sharded.  ValueError, before any device
    work: ``tsne_affinities``', ``n_iter`` < 1, an ``init`` of the wrong shape, dtype or device, a bad seed."""
    n, K, perp = _tsne_rows(xf, perplexity, metric, 'tsne')
    n_iter, lr, alpha, switch, seed = _tsne_optimiser(n_iter, learning_rate, early_exaggeration, exaggeration_iter, seed,
                                                      init, n, 'tsne')
    row_ptr, col, val, info = tsne_affinities(xf, perp, metric, block_cols, block_bytes)
    iso = info['isolated'].to(torch.uint8)
    return _tsne_result(row_ptr, col, val, iso, n, n_iter, lr, alpha, switch, seed, init, perp, metric, info['beta'])


# ----------------------------------------------------------------------------
# PCA and whitening by randomised subspace iteration (pca.hip)
# ----------------------------------------------------------------------------
PCA_LMAX = 512                   # GRL_PCA_LMAX of include/grl_hip.h
PCA_MAX_SWEEPS = 30              # GRL_PCA_MAX_SWEEPS
PCA_OFF_TOL = 2.0 ** -24         # a Jacobi run counts as converged when off <= PCA_OFF_TOL * |B|_F (it stops at 2^-26)
_PCA_PIVOT_CAUSE = {1: 'small', 2: 'nonfinite'}       # GRL_PCA_PIVOT_SMALL / _NONFINITE


def _pad32(v):
    return -(-v // 32) * 32


def _pca_pivot_tol(L):
    """A pivot at or below L * 2^-23 of the diagonal entry it started from (the row's own squared length) is within the
    rounding of the factorisation itself: the row is a combination of the rows before it as far as fp32 can tell."""
    return float(L) * 2.0 ** -23


def _pca_tail(L, dev):
    """One int32 block that a fit reads back once: the pivot record (8 words, GrlPcaRecord), the Jacobi info (4,
    GrlPcaEighInfo), sum |x_i|^2 and |mu|^2 (2 + 2 spare), then the L eigenvalues padded to a multiple of 32."""
    tail = torch.zeros(16 + _pad32(L), dtype=torch.int32, device=dev)
    tail[:5] = torch.tensor([0x7f800000, 0, -1, -1, 0], dtype=torch.int32)      # {+inf, no failure, no index, no call, 0 calls}
    return tail


def _pca_matrix(t, what, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
        raise ValueError('%s: %s must be a 2-d float32 tensor on a HIP device (got %s)'
                         % (what, name, '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t)
                            else type(t).__name__))
    return t


def _pca_orth(w, L, m, rec):
    """CholeskyQR2 in place on the rows of w [>= L, ld] (m columns used, ld % 32 == 0, the columns m.. zero): twice
    G = W W^T (the GEMM), G = R R^T (grl_pca_cholesky into the sticky record ``rec``), W <- R^-1 W (grl_pca_trsm)."""
    ld, Lp = w.shape[1], _pad32(L)
    g = _new((L, Lp), w)
    for _ in range(2):
        gemm(w, w, g, L, L, ld, lda=ld, ldw=ld, ldy=Lp, math=MATH_F32)
        _call('grl_pca_cholesky', ptr(g), Lp, L, _pca_pivot_tol(L), ptr(rec))
        _call('grl_pca_trsm', ptr(g), Lp, ptr(w), ld, L, m)


def _pca_shift(mu, c, rows, lam, scale, shift, cm):
    """The epilogue of a GEMM against the centred rows: cm = C mu (one GEMM row), scale = 1 / sqrt(lam) or 1, shift =
    -(cm * scale) (grl_pca_affine)."""
    dp = mu.shape[1]
    gemm(mu, c, cm, 1, rows, dp, math=MATH_F32)
    _call('grl_pca_affine', ptr(cm), ptr(lam), rows, ptr(scale), ptr(shift))


def _pca_wgrad(z, x, out, n, N, K, ldz):
    """out [N, K] = z^T x over the n rows: the deterministic slab-reduced weight-gradient GEMM in exact fp32."""
    d = _lib.GrlWgrad(ptr(z), ptr(x), ptr(out), None, n, N, K, ldz, K, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, MATH_F32, 0)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.grl_wgrad_workspace_floats(C.byref(d))), 4), dtype=torch.float32, device=z.device)
    d.workspace = ptr(ws)
    check(lib.grl_conv_wgrad_f32(C.byref(d), _lib.stream()), 'grl_conv_wgrad_f32')
    if _DEBUG_SYNC:
        _debug_sync('pca wgrad %s' % ((n, N, K),))


class _PcaFit(object):
    """The buffers and stages of one fit; ``tools/pca_rate.py`` times the stages one by one.  Everything is padded with
    zeros to what the GEMMs take (K % 32 == 0, ld % 4 == 0): q [Lp, dp], z [np, Lp], zt [Lp, np]."""

    def __init__(self, xp, n, d, L, dev):
        self.xp, self.n, self.d, self.L = xp, n, d, L
        self.dp, self.np_, self.Lp, self.L4 = xp.shape[1], _pad32(n), _pad32(L), (L + 3) // 4 * 4
        self.tail = _pca_tail(L, dev)
        self.rec = self.tail[:8]
        self.q = torch.zeros((self.Lp, self.dp), dtype=torch.float32, device=dev)
        self.z = torch.zeros((self.np_, self.Lp), dtype=torch.float32, device=dev)
        self.zt = torch.empty((self.Lp, self.np_), dtype=torch.float32, device=dev)
        self.cm, self.one, self.shift = (torch.zeros(self.Lp, dtype=torch.float32, device=dev) for _ in range(3))
        self.s = torch.empty(self.Lp, dtype=torch.float32, device=dev)
        self.mu = None

    def mean(self):
        """mu [1, dp]: cluster_centroids(xf, zeros, 1, 'mean')'s kernels (the padding columns come out +0)."""
        dev = self.xp.device
        labels = torch.zeros(self.n, dtype=torch.int32, device=dev)
        counts = torch.full((1,), self.n, dtype=torch.int32, device=dev)
        self.mu = _kmeans_update(self.xp, labels, counts, 1, 'mean')[0]

    def orth_q(self):
        _pca_orth(self.q, self.L, self.d, self.rec)

    def project(self):
        """z [n, L] = Xc Q^T = X Q^T - 1 (Q mu)^T (the GEMM's shift), and zt = its transpose."""
        _pca_shift(self.mu, self.q, self.L4, None, self.one, self.shift, self.cm)
        gemm(self.xp, self.q, self.z, self.n, self.L4, self.dp, ldy=self.Lp, shift=self.shift, math=MATH_F32)
        _call('grl_transpose', ptr(self.z), ptr(self.zt), self.np_, self.Lp, self.Lp)

    def orth_z(self):
        _pca_orth(self.zt, self.L, self.n, self.rec)

    def back(self):
        """q [L, d] = Z^T Xc = Z^T X - (Z^T 1) mu^T: the weight-gradient GEMM and the rank-one term."""
        _call('grl_pca_rowsum', ptr(self.zt), self.np_, self.L, self.n, ptr(self.s))
        _call('grl_transpose', ptr(self.zt), ptr(self.z), self.Lp, self.np_, self.np_)
        _pca_wgrad(self.z, self.xp, self.q, self.n, self.L4, self.dp, self.Lp)
        _call('grl_pca_rank1', ptr(self.q), self.dp, self.L, self.d, ptr(self.s), ptr(self.mu))

    def ritz_matrix(self):
        """b [L, Lp] = Z^T Z * (1 / (n - 1)) (after ``project``)."""
        import numpy as np
        inv = torch.full((self.Lp,), float(np.float32(1.0) / np.float32(self.n - 1)), dtype=torch.float32,
                         device=self.xp.device)
        b = _new((self.L, self.Lp), self.xp)
        gemm(self.zt, self.zt, b, self.L, self.L, self.np_, lda=self.np_, ldw=self.np_, ldy=self.Lp, scale=inv,
             math=MATH_F32)
        return b

    def eigh(self, b):
        """lam (in the tail block) and vt [Lp, Lp] of b, destroyed (grl_pca_eigh)."""
        vtw = _new((self.L, self.Lp), b)
        vt = torch.zeros((self.Lp, self.Lp), dtype=torch.float32, device=b.device)
        lam = self.tail[16:].view(torch.float32)
        _call('grl_pca_eigh', ptr(b), self.Lp, ptr(vtw), self.Lp, self.L, ptr(lam), ptr(vt), self.Lp, ptr(self.tail[8:12]))
        return lam, vt

    def components(self, vt, r):
        """The first r rows of V^T Q as [r, dp], signs fixed (grl_pca_sign)."""
        qt = _new((self.dp, self.Lp), self.q)
        _call('grl_transpose', ptr(self.q), ptr(qt), self.Lp, self.dp, self.dp)
        c = _new((r, self.dp), self.q)
        gemm(vt, qt, c, r, self.dp, self.Lp, math=MATH_F32)
        _call('grl_pca_sign', ptr(c), self.dp, r, self.d)
        return c

    def sums(self):
        """sum_i |x_i|^2 and |mu|^2 into the tail block: grl_row_sqnorm, the first folded in the wave order."""
        sq = _new((self.n,), self.xp)
        f = self.tail[12:16].view(torch.float32)
        _call('grl_row_sqnorm', ptr(self.xp), ptr(sq), self.n, self.dp, self.dp)
        _call('grl_pca_rowsum', ptr(sq), self.n, 1, self.n, ptr(f))
        _call('grl_row_sqnorm', ptr(self.mu), ptr(f[1:]), 1, self.dp, self.dp)


def _pca_raise(what, status, index, call, L):
    if _PCA_PIVOT_CAUSE.get(status) == 'nonfinite':
        raise _lib.GrlHipError('%s: a Cholesky pivot is not finite (pivot %d of factorisation %d): the features hold NaN '
                               'or infinite values -- remove the non-finite rows' % (what, index, call))
    raise _lib.GrlHipError('%s: Cholesky pivot %d of factorisation %d is not positive in fp32: L = n_components + '
                           'oversample = %d is above the numerical rank of the centred features -- lower n_components / '
                           'oversample' % (what, index, call, L))


class Pca(object):
    """The result of ``pca``, everything on the device:

      mean                     float32 [d]: cluster_centroids(xf, zeros, 1, 'mean')[0][0] bit for bit
      components               float32 [r, d], orthonormal rows, the entry of largest magnitude of each positive
      explained_variance       float32 [r] descending; explained_variance_ratio = it * float32(1 / total_variance)
      total_variance           float: (sum |x_i|^2 - n |mean|^2) / (n - 1)
      n_samples, n_iter, seed, oversample
      sweeps                   Jacobi sweeps of the Rayleigh-Ritz eigensolve;  off: the off-diagonal norm it left
      min_pivot                the smallest Cholesky pivot of the fit relative to its Gram matrix's largest diagonal"""

    def __init__(self, mu, cpad, lam, d, total, n, n_iter, seed, oversample, sweeps, off, min_pivot, lam_host):
        self._mu, self._cpad, self._d, self._lam_host = mu, cpad, d, lam_host
        self.mean = mu[0, :d]
        self.components = cpad[:, :d] if cpad.shape[1] == d else cpad[:, :d].contiguous()
        self.explained_variance = lam
        self.total_variance, self.n_samples, self.n_iter, self.seed, self.oversample = total, n, n_iter, seed, oversample
        self.sweeps, self.off, self.min_pivot = sweeps, off, min_pivot
        self.explained_variance_ratio = None
        self._aff = {}
        self._ct = None

    def _rows(self, x, what, width, name):
        _pca_matrix(x, what, name)
        if x.shape[1] != width:
            raise ValueError('%s: %s has %d columns, the fit has %d' % (what, name, x.shape[1], width))
        return _pad_features(x)

    def affine(self, whiten=False):
        """(scale, shift) float32 [r] of the transform GEMM: scale_i = 1 / sqrt(lambda_i) with ``whiten`` else 1,
        shift_i = -(C mu)_i * scale_i.  ValueError: ``whiten`` with a kept variance that is <= 0 or not finite."""
        import math
        whiten = bool(whiten)
        if whiten and not all(math.isfinite(v) and v > 0 for v in self._lam_host):
            raise ValueError('Pca: whiten needs every kept explained_variance finite and > 0 (the smallest kept one is '
                             '%r): lower n_components' % (min(self._lam_host),))
        if whiten not in self._aff:
            r = self._cpad.shape[0]
            cm, scale, shift = (_new((r,), self._cpad) for _ in range(3))
            _pca_shift(self._mu, self._cpad, r, self.explained_variance if whiten else None, scale, shift, cm)
            self._aff[whiten] = (scale, shift)
        return self._aff[whiten]

    def transform(self, x, whiten=False):
        """Y [rows, r] = (x - mean) C^T, column i times 1 / sqrt(lambda_i) with ``whiten``: one
        ``gemm(x, C, scale=scale, shift=shift)`` with ``affine(whiten)``, exact fp32 whatever the math mode.  Any rows."""
        xp = self._rows(x, 'Pca.transform', self._d, 'x')
        scale, shift = self.affine(whiten)
        rows, r = xp.shape[0], self._cpad.shape[0]
        y = _new((rows, r), xp)
        if rows:
            gemm(xp, self._cpad, y, rows, r, xp.shape[1], scale=scale, shift=shift, math=MATH_F32)
        return y

    def inverse_transform(self, y, whiten=False):
        """X^ [rows, d] = y C + mean (y times sqrt(lambda) first when it was whitened): one GEMM with the mean as shift."""
        r, d = self._cpad.shape[0], self._d
        y = self._rows(y, 'Pca.inverse_transform', r, 'y')
        rows, rp = y.shape[0], y.shape[1]
        if whiten:
            self.affine(True)
            yw = torch.zeros_like(y)
            _call('grl_pca_colscale', ptr(y), rp, rows, r, ptr(self.explained_variance), ptr(yw), rp)
            y = yw
        if self._ct is None:
            dp = self._cpad.shape[1]
            crows = torch.zeros((rp, dp), dtype=torch.float32, device=y.device)
            crows[:r] = self._cpad
            self._ct = _new((dp, rp), y)
            _call('grl_transpose', ptr(crows), ptr(self._ct), rp, dp, dp)
        out = _new((rows, d), y)
        if rows:
            gemm(y, self._ct, out, rows, d, rp, shift=self._mu, math=MATH_F32)
        return out

    def tsne_init(self, x):
        """scikit-learn's ``init='pca'`` start of t-SNE, float32 [rows, 2]: the first two transformed columns divided by
        the population standard deviation of the first and multiplied by 1e-4 (grl_pca_tsne_init); use as
        ``tsne(xf, init=pca(xf, 2).tsne_init(xf))``.  Needs n_components >= 2."""
        if self._cpad.shape[0] < 2:
            raise ValueError('Pca.tsne_init: needs n_components >= 2 (the fit kept %d)' % self._cpad.shape[0])
        xp = self._rows(x, 'Pca.tsne_init', self._d, 'x')
        rows = xp.shape[0]
        if rows < 1:
            raise ValueError('Pca.tsne_init: x has no rows')
        shift = self.affine(False)[1]
        y = _new((rows, 2), xp)
        gemm(xp, self._cpad, y, rows, 2, xp.shape[1], shift=shift, math=MATH_F32)
        out = torch.empty_like(y)
        _call('grl_pca_tsne_init', ptr(y), 2, rows, ptr(out))
        return out


def _pca_args(xf, n_components, oversample, n_iter, seed, what):
    """The checks of ``pca`` that need no device work: (n, d, r, p, q, seed)."""
    _pca_matrix(xf, what, 'xf')
    n, d = int(xf.shape[0]), int(xf.shape[1])
    r = _int_arg(n_components, 1, None, what, 'n_components')
    p = _int_arg(oversample, 0, None, what, 'oversample')
    q = _int_arg(n_iter, 0, None, what, 'n_iter')
    seed = _int_arg(seed, 0, None, what, 'seed')
    if n < 2:
        raise ValueError('%s: needs n >= 2 samples (got %s)' % (what, tuple(xf.shape)))
    if r + p > min(n - 1, d) or r + p > PCA_LMAX:
        raise ValueError('%s: L = n_components + oversample = %d must be at most min(n - 1, d, %d) = %d: lower '
                         'n_components / oversample' % (what, r + p, PCA_LMAX, min(n - 1, d, PCA_LMAX)))
    return n, d, r, p, q, seed


def pca(xf, n_components, oversample=10, n_iter=4, seed=0):
    """PCA of the rows of ``xf`` [n, d] on the device by randomised subspace iteration, as a ``Pca``: the state is
    O((n + d) L + L^2) with L = n_components + oversample -- no d x d covariance, no n x n Gram matrix, no centred copy
    (every product with the centred rows is the product with ``xf`` and a rank-one term).  The start is
    Generator(PCG64(seed)).standard_normal((L, d)) as float32 from the host, orthonormalised by CholeskyQR2; ``n_iter``
    power iterations with both halves orthonormalised; Rayleigh-Ritz with the Jacobi eigensolver.  The tall products are
    ``gemm`` and the slab-reduced weight-gradient GEMM in exact fp32 whatever ``set_math`` says; everything between is
    pca.hip.  One read-back, at the end.  The same bits on every run.  Not sharded: every rank computes the same result
    and issues no collective.  ValueError, before any device work: ``xf`` not a 2-d float32 device tensor, n < 2,
    arguments that are not integers (a bool is none) or out of range, L > min(n - 1, d, 512).  GrlHipError: a Cholesky
    pivot that is not positive (L above the numerical rank: lower n_components / oversample) or not finite (remove the
    non-finite rows), a Jacobi run that did not converge in 30 sweeps."""
    import numpy as np
    what = 'pca'
    n, d, r, p, q, seed = _pca_args(xf, n_components, oversample, n_iter, seed, what)
    L, dev = r + p, xf.device
    fit = _PcaFit(_pad_features(xf), n, d, L, dev)
    fit.mean()
    q0 = np.random.Generator(np.random.PCG64(seed)).standard_normal((L, d)).astype(np.float32)
    fit.q[:L, :d] = torch.from_numpy(q0).to(dev)
    fit.orth_q()
    for _ in range(q):
        fit.project()
        fit.orth_z()
        fit.back()
        fit.orth_q()
    fit.project()
    lam, vt = fit.eigh(fit.ritz_matrix())
    cpad = fit.components(vt, r)
    fit.sums()
    host = fit.tail.cpu()                                   # the one read-back
    status, index, call = int(host[1]), int(host[2]), int(host[3])
    if status:
        _pca_raise(what, status, index, call, L)
    hf = host.view(torch.float32)
    min_pivot, sweeps, off, fro = float(hf[0]), int(host[8]), float(hf[9]), float(hf[10])
    if not off <= PCA_OFF_TOL * fro:
        raise _lib.GrlHipError('%s: the Jacobi eigensolver left an off-diagonal norm of %g on a matrix of norm %g after %d '
                               'sweeps (converged is <= 2^-24 of the norm): the features hold non-finite values -- remove '
                               'the non-finite rows -- or the Rayleigh-Ritz matrix is not symmetric' % (what, off, fro, sweeps))
    total = (float(hf[12]) - n * float(hf[13])) / (n - 1)
    out = Pca(fit.mu, cpad, lam[:r].clone(), d, total, n, q, seed, p, sweeps, off, min_pivot,
              [float(v) for v in hf[16:16 + r]])
    ratio = torch.empty_like(lam)
    _call('grl_axpby', ptr(lam), None, ptr(ratio), float(np.float32(1.0) / np.float32(total)) if total > 0 else float('nan'),
          0.0, lam.numel())
    out.explained_variance_ratio = ratio[:r].clone()
    return out


def pca_eigh(b):
    """The eigendecomposition of the symmetric ``b`` [L, L], L <= 512, by the fit's cyclic Jacobi kernel (grl_pca_eigh:
    fixed round-robin pairing, at most 30 sweeps): ``(lam [L] descending, v [L, L] with b = v diag(lam) v^T, sweeps)``.
    Only the upper triangle of ``b`` is read.  GrlHipError when the run did not converge."""
    what = 'pca_eigh'
    _pca_matrix(b, what, 'b')
    L = int(b.shape[0])
    if b.shape[1] != L or not 1 <= L <= PCA_LMAX:
        raise ValueError('%s: b must be square with 1 <= L <= %d (got %s)' % (what, PCA_LMAX, tuple(b.shape)))
    Lp = _pad32(L)
    a = torch.zeros((L, Lp), dtype=torch.float32, device=b.device)
    a[:, :L] = b
    vtw, vt = _new((L, Lp), b), _new((L, Lp), b)
    lam = _new((L,), b)
    info = torch.zeros(4, dtype=torch.int32, device=b.device)
    _call('grl_pca_eigh', ptr(a), Lp, ptr(vtw), Lp, L, ptr(lam), ptr(vt), Lp, ptr(info))
    host = info.cpu()
    sweeps, off, fro = int(host[0]), float(host.view(torch.float32)[1]), float(host.view(torch.float32)[2])
    if not off <= PCA_OFF_TOL * fro:
        raise _lib.GrlHipError('%s: off-diagonal norm %g of a matrix of norm %g after %d sweeps: not converged (b must be '
                               'finite and symmetric)' % (what, off, fro, sweeps))
    return lam, vt[:, :L].t().contiguous(), sweeps


class PcaOrth(tuple):
    """``(q, min_pivot)`` of ``pca_orthonormalize`` with the pivot record's ``status`` (0 = fine, 'small', 'nonfinite')
    and the ``index`` and ``call`` (0 or 1) of the first failing pivot."""

    def __new__(cls, q, min_pivot, status, index, call):
        self = tuple.__new__(cls, (q, min_pivot))
        self.status, self.index, self.call = status, index, call
        return self


def pca_orthonormalize(w):
    """The rows of ``w`` [L, m], L <= min(m, 512), orthonormalised by the fit's CholeskyQR2 (twice: Gram matrix by the
    GEMM, grl_pca_cholesky, grl_pca_trsm): ``(q [L, m], min_pivot)``, q = T w with T lower triangular, min_pivot the
    smallest pivot relative to the Gram matrix's largest diagonal entry over both passes.  Dependent rows do not raise:
    the result's ``status`` is 'small' (or 'nonfinite'), ``index`` the first failing pivot (one at or below L * 2^-23 of
    its row's own squared length), and q is finite for finite input -- the rows from ``index`` on orthogonal to those before, not normalised."""
    what = 'pca_orthonormalize'
    _pca_matrix(w, what, 'w')
    L, m = int(w.shape[0]), int(w.shape[1])
    if not 1 <= L <= min(m, PCA_LMAX):
        raise ValueError('%s: w must be [L, m] with 1 <= L <= min(m, %d) (got %s)' % (what, PCA_LMAX, tuple(w.shape)))
    buf = torch.zeros((L, _pad32(m)), dtype=torch.float32, device=w.device)
    buf[:, :m] = w
    tail = _pca_tail(1, w.device)
    _pca_orth(buf, L, m, tail[:8])
    host = tail[:8].cpu()
    return PcaOrth(buf[:, :m].contiguous(), float(host.view(torch.float32)[0]), _PCA_PIVOT_CAUSE.get(int(host[1]), 0),
                   int(host[2]), int(host[3]))


# ----------------------------------------------------------------------------
# diffusion (manifold ranking) on the gallery's mutual-kNN graph (diffusion.hip)
# ----------------------------------------------------------------------------
DIFFUSION_K_MAX = 128
DIFFUSION_GAMMA_MAX = 8


class DiffusionGraph(object):
    """The symmetric, degree-normalised mutual-kNN graph of ``diffusion_graph`` in a fixed-width (ELL) layout: ``idx``
    int32 [n, k] (row i's k nearest other rows in ``search``'s order, -1 = padding), ``weight`` float32 [n, k] (S of
    (I - alpha S) f = y: a / (sqrt(deg_i) sqrt(deg_j)) with a = min(w_ij, w_ji) on a mutual edge, 0 elsewhere) and
    ``deg`` float32 [n] (the row sums of a), all on the device; ``n``, ``k``, ``gamma``; ``n_edges`` = the non-zero slots
    (every undirected edge counts twice), ``n_isolated`` = the rows without one."""

    def __init__(self, idx, weight, deg, n, k, gamma):
        self.idx, self.weight, self.deg = idx, weight, deg
        self.n, self.k, self.gamma = n, k, gamma
        self.n_edges = int(torch.count_nonzero(weight)) if n else 0
        self.n_isolated = int((deg == 0).sum()) if n else 0

    def __repr__(self):
        return 'DiffusionGraph(n=%d, k=%d, gamma=%d, n_edges=%d, n_isolated=%d)' % (self.n, self.k, self.gamma,
                                                                                    self.n_edges, self.n_isolated)


def _diffusion_int(v, lo, hi, what, name):
    return _int_arg(v, lo, hi, what, name, 'in %d..' % lo if hi >= _INT_MAX else None)


def _diffusion_graph_args(k, gamma, what):
    return (_diffusion_int(k, 1, DIFFUSION_K_MAX, what, 'k'), _diffusion_int(gamma, 1, DIFFUSION_GAMMA_MAX, what, 'gamma'))


def _diffusion_solve_args(alpha, n_iter, what):
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0.0 <= alpha < 1.0:    # (NaN fails both)
        raise ValueError('%s: alpha must be a number in [0, 1) (got %r)' % (what, alpha))
    if not 0.0 <= float(torch.tensor(float(alpha), dtype=torch.float32)) < 1.0:
        raise ValueError('%s: alpha must stay below 1 in float32 (got %r)' % (what, alpha))
    return float(alpha), _diffusion_int(n_iter, 0, _INT_MAX, what, 'n_iter')


def _diffusion_kq(kq, k, what):
    kq = _diffusion_int(kq, 1, DIFFUSION_K_MAX, what, 'kq')
    if kq > k:
        raise ValueError('%s: kq must not exceed k (got kq = %d, k = %d)' % (what, kq, k))
    return kq


def _diffusion_rows(t, what, name):
    """``t`` as a contiguous float32 device matrix, or ValueError."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2):
        raise ValueError('%s: %s must be a float32 matrix on a HIP device (got %s)'
                         % (what, name, getattr(t, 'device', type(t))))
    return t.contiguous().view(t.shape[0], int(torch.Size(t.shape[1:]).numel()))


def _diffusion_metric(metric, what):
    if isinstance(metric, VerifyMetric):
        raise ValueError('%s: a verify_metric is the signed logit of modified query rows against gallery rows, not a '
                         "distance between two samples of one set; the graph is built by 'cosine'" % what)
    if metric != 'cosine':
        raise ValueError("%s: metric must be 'cosine' (got %r): the edge weights are powers of the cosine similarity"
                         % (what, metric))


def _diffusion_check_graph(graph, what):
    if not isinstance(graph, DiffusionGraph):
        raise ValueError('%s: graph must be the DiffusionGraph of diffusion_graph (got %r)' % (what, type(graph)))


def diffusion_graph(gf, k=50, gamma=3, metric='cosine', block_cols=None, block_bytes=None):
    """The mutual-kNN graph of the rows of ``gf`` [n, d] (unit norm) for ``diffusion_solve`` / ``diffusion_search``, as a
    ``DiffusionGraph``.  ``search(gf, gf, k + 1)`` by cosine gives every row's list; the row itself is dropped from it
    (the last entry when duplicates that tie before it pushed the row out of its own list).  Weight of a neighbour:
    w = max(q . g, 0) ** gamma by gamma - 1 products (``gamma`` an integer in 1..8, as ``expand_features`` restricts its
    alpha); an edge exists where i and j are in each other's lists and carries min(w_ij, w_ji), which makes the matrix
    symmetric bit for bit; S = D^-1/2 A D^-1/2.  1 <= k <= 128.  Memory: the lists and O(n k); the n x n matrix is never
    built (``block_cols`` / ``block_bytes`` are ``search``'s).  Not sharded: under torch.distributed ``search`` is
    collective and returns identical lists on every rank, and every rank builds the full, identical graph, as ``cluster``
    does."""
    what = 'diffusion_graph'
    k, gamma = _diffusion_graph_args(k, gamma, what)
    _diffusion_metric(metric, what)
    gf = _diffusion_rows(gf, what, 'gf')
    n, dev = gf.shape[0], gf.device
    sdist = sidx = None
    if n:
        sdist, sidx = search(gf, gf, k + 1, block_cols=block_cols, block_bytes=block_bytes)
    idx = torch.full((n, k), -1, dtype=torch.int32, device=dev)           # (after the search: its block is gone by now)
    weight = torch.zeros((n, k), dtype=torch.float32, device=dev)
    deg = torch.zeros((n,), dtype=torch.float32, device=dev)
    if n:
        _call('grl_diffusion_mutual', ptr(sidx), ptr(sdist), k + 1, n, k, gamma, ptr(idx), ptr(weight), k, ptr(deg))
    return DiffusionGraph(idx, weight, deg, n, k, gamma)


def _diffusion_block(graph, seed_idx, seed_val, seed_gamma, alpha, n_iter, negate):
    """One block of queries: scatter the seeds into y [n][B], solve, and return x transposed, [B][n] (negated for the
    ranking kernels).  seed_gamma 0: ``seed_val`` holds the values; >= 1: search's cosine distances."""
    n, B, dev = graph.n, seed_idx.shape[0], graph.idx.device
    lib = _lib.load()
    y = torch.empty((n, B), dtype=torch.float32, device=dev)
    x = torch.empty((n, B), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.grl_diffusion_workspace_floats(n, B),), dtype=torch.float32, device=dev)
    _call('grl_diffusion_seed', ptr(seed_idx), ptr(seed_val), seed_idx.shape[1], B, seed_idx.shape[1], n, seed_gamma,
          ptr(y))
    _call('grl_diffusion_solve', ptr(graph.idx), ptr(graph.weight), graph.k, n, graph.k, ptr(y), B, alpha, n_iter, ptr(x),
          ptr(ws))
    del y, ws
    out = torch.empty((B, n), dtype=torch.float32, device=dev)
    _call('grl_diffusion_transpose', ptr(x), n, B, 1 if negate else 0, ptr(out), n)
    return out


def diffusion_solve(graph, seed_idx, seed_val, alpha=0.99, n_iter=20):
    """``f`` float32 [nq_block, n]: row q solves (I - alpha S) f = y_q on ``graph`` for y_q = ``seed_val[q]`` at the nodes
    ``seed_idx[q]`` (int64 [nq_block, kq] on the device, -1 = padding, distinct per row) and 0 elsewhere, by exactly
    ``n_iter`` iterations of plain conjugate gradients from x0 = 0 (the matrix is symmetric positive definite: S's
    spectrum lies in [-1, 1] and 0 <= alpha < 1).  All columns advance together, [n][nq_block] node-major, and are
    independent; a column whose residual is 0 (or whose p . Ap is not positive and finite) freezes, so a zero seed column
    stays zero and alpha = 0 returns y exactly.  n_iter = 0 returns zeros.  Every sum has a fixed order
    (tests/diffusion_ref.py reproduces the result bit for bit, and two calls give the same bits).  This is the low-level
    solve for one block of queries: memory is 5 n nq_block floats."""
    what = 'diffusion_solve'
    _diffusion_check_graph(graph, what)
    alpha, n_iter = _diffusion_solve_args(alpha, n_iter, what)
    if not (torch.is_tensor(seed_idx) and seed_idx.is_cuda and seed_idx.dtype == torch.int64 and seed_idx.dim() == 2):
        raise ValueError('%s: seed_idx must be an int64 device matrix [nq_block, kq]' % what)
    if not (torch.is_tensor(seed_val) and seed_val.is_cuda and seed_val.dtype == torch.float32
            and tuple(seed_val.shape) == tuple(seed_idx.shape)):
        raise ValueError('%s: seed_val must be a float32 device matrix of seed_idx\'s shape' % what)
    B, n = seed_idx.shape[0], graph.n
    if B == 0 or n == 0 or seed_idx.shape[1] == 0:
        return torch.zeros((B, n), dtype=torch.float32, device=graph.idx.device)
    return _diffusion_block(graph, seed_idx.contiguous(), seed_val.contiguous(), 0, alpha, n_iter, False)


def _diffusion_query_block(query_block, block_bytes, n, nq, vectors, what):
    """Queries per block: ``query_block``, or what fits ``block_bytes`` (GRL_SEARCH_BLOCK_BYTES) counting ``vectors``
    [n][B] float arrays -- a multiple of 64 from 256 on, which keeps the 16-byte accesses of the state."""
    if query_block is not None:
        return _diffusion_int(query_block, 1, _INT_MAX, what, 'query_block')
    B = max(1, min(nq, _block_budget(block_bytes) // (4 * vectors * max(n, 1))))
    return B // 64 * 64 if B >= 256 else B


def _diffusion_prepare(qf, gf, graph, kq, alpha, n_iter, k, gamma, what):
    if graph is None:
        k, gamma = _diffusion_graph_args(k, gamma, what)
    else:
        _diffusion_check_graph(graph, what)
        k, gamma = graph.k, graph.gamma
    kq = _diffusion_kq(kq, k, what)
    alpha, n_iter = _diffusion_solve_args(alpha, n_iter, what)
    qf, gf = _diffusion_rows(qf, what, 'qf'), _diffusion_rows(gf, what, 'gf')
    if qf.shape[1] != gf.shape[1]:
        raise ValueError('qf and gf have different feature sizes (%d, %d)' % (qf.shape[1], gf.shape[1]))
    if graph is not None and graph.n != gf.shape[0]:
        raise ValueError('%s: the graph has %d nodes, gf has %d rows' % (what, graph.n, gf.shape[0]))
    return qf, gf, kq, alpha, n_iter, k, gamma


def _diffusion_blocks(qf, gf, graph, kq, alpha, n_iter, B, block_bytes=None):
    """(q0, q1, the [q1 - q0][n] block of -f) per block of ``B`` queries.  The seeds are ``search(qf, gf, kq)`` with no
    junk rule: that rule belongs to the final ranking only, as in re-ranking."""
    sdist, sidx = search(qf, gf, kq, block_bytes=block_bytes)
    for q0 in range(0, qf.shape[0], B):
        q1 = min(q0 + B, qf.shape[0])
        yield q0, q1, _diffusion_block(graph, sidx[q0:q1].contiguous(), sdist[q0:q1].contiguous(), graph.gamma, alpha,
                                       n_iter, True)


def diffusion_search(qf, gf, k_out, graph=None, kq=10, alpha=0.99, n_iter=20, k=50, gamma=3, exclude=None,
                     query_block=None, block_bytes=None):
    """Diffusion re-ranking (Zhou et al., "Ranking on data manifolds"; Iscen et al., CVPR 2017): each query's ``k_out``
    best gallery entries under the scores f of (I - alpha S) f = y, ``(score [nq, k_out] float32 = -f, idx [nq, k_out]
    int64)`` on the device, ascending in -f, ties to the smaller gallery index, padded as ``search`` pads (index -1,
    +inf).  S is ``graph`` (``diffusion_graph(gf, k, gamma)`` when None; a prebuilt graph is reused and brings its own k
    and gamma); y_q holds max(q . g, 0) ** gamma at the query's ``kq`` nearest gallery rows (kq <= k) and 0 elsewhere; the
    solve is ``diffusion_solve``'s (``n_iter`` conjugate-gradient iterations; 0 leaves f = 0 and the ranking is the index
    order).  ``exclude`` has ``search``'s meaning and is applied to the final ranking only.  Queries are processed in
    blocks of ``query_block`` columns (default: what fits ``block_bytes`` / GRL_SEARCH_BLOCK_BYTES, counting the four
    CG vectors and the transposed block); every block size gives the same bits.  Memory is O(n k + n B): no nq x n and no
    n x n tensor is allocated.  Not sharded: under torch.distributed every rank computes the full, identical result, as
    ``cluster`` does (the ``search`` calls inside are collective)."""
    what = 'diffusion_search'
    if not 1 <= int(k_out) <= SEARCH_K_MAX:
        raise ValueError('%s: k_out must be in 1..%d (got %r)' % (what, SEARCH_K_MAX, k_out))
    k_out = int(k_out)
    qf, gf, kq, alpha, n_iter, k, gamma = _diffusion_prepare(qf, gf, graph, kq, alpha, n_iter, k, gamma, what)
    nq, n, dev = qf.shape[0], gf.shape[0], qf.device
    junk = _junk_ids(exclude, nq, n, dev)
    top = _TopK(nq, k_out, dev)
    if nq and n:
        B = _diffusion_query_block(query_block, block_bytes, n, nq, 5, what)
        if graph is None:
            graph = diffusion_graph(gf, k, gamma, block_bytes=block_bytes)
        for q0, q1, d in _diffusion_blocks(qf, gf, graph, kq, alpha, n_iter, B, block_bytes):
            top.push(d, n, n, 0, junk=junk, rows=(q0, q1))
    return top.result()


def diffusion_metrics_streaming(qf, gf, q_pids, g_pids, q_camids, g_camids, graph=None, kq=10, alpha=0.99, n_iter=20,
                                k=50, gamma=3, max_rank=100, query_block=None, block_bytes=None):
    """``rank_metrics(rank_rows(-f), ...)`` of the diffusion scores of ``diffusion_search`` without the nq x n matrix:
    (cmc[max_rank] float32, mAP float) of eva_functions.evaluate.  Per block of ``query_block`` queries the [B][n] block of
    -f is ranked by ``rank_rows`` and scored by grl_rank_metrics (the junk rule: same pid AND camera); the per-query (first
    match rank, #matches, AP) are concatenated and averaged once, so every block size gives the same result.  The default
    block also counts the block's int32 argsort.  Not sharded (see ``diffusion_search``)."""
    what = 'diffusion_metrics_streaming'
    qf, gf, kq, alpha, n_iter, k, gamma = _diffusion_prepare(qf, gf, graph, kq, alpha, n_iter, k, gamma, what)
    nq, n, dev = qf.shape[0], gf.shape[0], qf.device
    qp, qc = _ids(q_pids, nq, 'q_pids', dev), _ids(q_camids, nq, 'q_camids', dev)
    gp, gc = _ids(g_pids, n, 'g_pids', dev), _ids(g_camids, n, 'g_camids', dev)
    first = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    nhit = torch.zeros(nq, dtype=torch.int32, device=dev)
    ap = torch.zeros(nq, dtype=torch.float64, device=dev)
    if nq and n:
        B = _diffusion_query_block(query_block, block_bytes, n, nq, 6, what)
        if graph is None:
            graph = diffusion_graph(gf, k, gamma, block_bytes=block_bytes)
        for q0, q1, d in _diffusion_blocks(qf, gf, graph, kq, alpha, n_iter, B, block_bytes):
            order = rank_rows(d)
            _call('grl_rank_metrics', ptr(order), n, ptr(qp[q0:q1]), ptr(qc[q0:q1]), ptr(gp), ptr(gc), q1 - q0, n,
                  ptr(first[q0:q1]), ptr(nhit[q0:q1]), ptr(ap[q0:q1]))
    return _cmc_map(first, nhit, ap, n, max_rank)


# ----------------------------------------------------------------------------
# tracklet set distances over clip features (setdist.hip)
# ----------------------------------------------------------------------------
SET_REDUCE = {'min': 0, 'mean': 1, 'chamfer': 2, 'hausdorff': 3}     # GRL_SET_* of include/grl_hip.h
SET_METRICS = ('cosine', 'euclidean')
SET_MAX_CLIPS = 1024                                                  # GRL_SET_MAX_CLIPS


def _set_args(reduce, metric, what):
    if reduce not in SET_REDUCE:
        raise ValueError("%s: reduce must be 'min', 'mean', 'chamfer' or 'hausdorff' (got %r)" % (what, reduce))
    if metric not in SET_METRICS:
        raise ValueError("%s: metric must be 'cosine' or 'euclidean' (got %r)" % (what, metric))


class TrackletSet(object):
    """``n`` tracklets as their clips: ``clips`` [N, d] float32 on the device, the rows of a tracklet consecutive, and
    ``counts`` [n], the clips per tracklet (1 .. 1024 each, N in all).  ``ptr`` (numpy int64 [n + 1]) / ``ptr_dev`` (the
    same on the device): tracklet t owns the rows ptr[t] .. ptr[t + 1].  The rows are zero-padded to a multiple of 32
    features when d is not one (``_pad_features``: +0 to every dot product and norm); ``d`` stays the width given.
    ValueError: counts that are not integers in 1..1024 or do not add up to N (checked before the device is looked at)."""

    def __init__(self, clips, counts):
        import numpy as np
        if not (torch.is_tensor(clips) and clips.dim() == 2):
            raise ValueError('TrackletSet: clips must be a 2-d tensor [N, d] (got %s)'
                             % (tuple(clips.shape) if torch.is_tensor(clips) else type(clips).__name__,))
        c = np.asarray(counts)
        if c.ndim != 1 or (c.size and c.dtype.kind not in 'iu'):
            raise ValueError('TrackletSet: counts must be a list of integers (got %r)' % (counts,))
        c = c.astype(np.int64)
        if c.size and c.min() < 1:
            raise ValueError('TrackletSet: every tracklet needs at least one clip (tracklet %d has %d)'
                             % (int(c.argmin()), int(c.min())))
        if c.size and c.max() > SET_MAX_CLIPS:
            raise ValueError('TrackletSet: a tracklet may have at most %d clips (tracklet %d has %d)'
                             % (SET_MAX_CLIPS, int(c.argmax()), int(c.max())))
        if int(c.sum()) != clips.shape[0]:
            raise ValueError('TrackletSet: the counts add up to %d clips, clips has %d rows' % (int(c.sum()), clips.shape[0]))
        require_device(clips, 'clips')
        self.n, self.d = int(c.size), int(clips.shape[1])
        self.clips = _pad_features(clips)
        self.counts = c
        self.ptr = np.zeros(self.n + 1, np.int64)
        np.cumsum(c, out=self.ptr[1:])
        self.ptr_dev = torch.from_numpy(self.ptr).to(clips.device)

    def mean_rows(self):
        """[n, d]: the mean of every tracklet's clips through grl_group_mean, one call per tracklet -- ``rows_mean`` of
        its rows, the row dense-mode evaluation ranks by today."""
        x, w = self.clips, self.clips.shape[1]
        y = _new((self.n, w), x)
        for t in range(self.n):
            a, b = int(self.ptr[t]), int(self.ptr[t + 1])
            _call('grl_group_mean', ptr(x[a:b]), ptr(y[t:]), 1, b - a, w, w, C.c_float(1.0), 0)
        return y if w == self.d else y[:, :self.d].contiguous()


def _set_ranges(ptr_, t0, t1, cap):
    """[t0, t1) cut into ranges of whole tracklets of at most ``cap`` clips each (one tracklet where it alone has more)."""
    import numpy as np
    out = []
    while t0 < t1:
        e = int(np.searchsorted(ptr_, ptr_[t0] + cap, side='right')) - 1
        e = min(max(e, t0 + 1), t1)
        out.append((t0, e))
        t0 = e
    return out


class _SetBlocks(_BlockSource):
    """Column blocks of the tracklet x tracklet set distance of ``qset`` against the tracklets [lo, hi) of ``gset``: a
    ``_BlockSource`` with spans in TRACKLET columns.  No tracklet is ever cut.  Without ``block_cols``
    a span takes as many whole gallery tracklets as keep the [nq, c1 - c0] output block within ``block_bytes``
    (GRL_SEARCH_BLOCK_BYTES).  Inside ``block`` the clip-level work is tiled over ranges of whole query tracklets and whole
    gallery tracklets whose clip x clip scratch stays within ``block_bytes`` too (a pair of tracklets that alone exceeds it
    is one tile: at most 4 MiB): per tile one fp32 distance GEMM of the clip rows into the scratch (NEGDOT / EUCLID, the
    entries of cosin_dist / pairwise_distance_tensor of the clip tensors, bit for bit) and one grl_setdist_block that folds
    every tracklet pair's cell into its entry of the block.  A cell's value does not depend on the tiling (include/grl_hip.h),
    so neither does a block.  The 'euclidean' norms come once per set from grl_row_sqnorm."""

    def __init__(self, qset, gset, reduce='chamfer', metric='cosine', block_cols=None, block_bytes=None, lo=0, hi=None):
        _set_args(reduce, metric, '_SetBlocks')
        if qset.clips.shape[1] != gset.clips.shape[1]:
            raise ValueError('qset and gset have different feature sizes (%d, %d)' % (qset.d, gset.d))
        hi = gset.n if hi is None else hi
        self.qset, self.gset, self.reduce, self.metric = qset, gset, SET_REDUCE[reduce], metric
        self.qf, self.nq, self.ng, self.lo = qset.clips, qset.n, gset.n, lo
        self.budget = _block_budget(block_bytes)
        self._cut(lo, hi, block_cols, block_bytes, granule=None)      # whole tracklets: no rounding, no floor of 256
        self.scratch = None
        self.rn = self.cn = None
        if metric == 'euclidean' and self.spans and self.nq:
            k = self.qf.shape[1]
            g0, g1 = int(gset.ptr[lo]), int(gset.ptr[hi])
            self.rn, self.cn, self.cn0 = _new((qset.clips.shape[0],), self.qf), _new((g1 - g0,), self.qf), g0
            _call('grl_row_sqnorm', ptr(self.qf), ptr(self.rn), qset.clips.shape[0], k, k)
            _call('grl_row_sqnorm', ptr(gset.clips[g0:g1]), ptr(self.cn), g1 - g0, k, k)

    def tiles(self, c0, c1):
        """(a0, a1, b0, b1): the tracklet ranges of the GEMM tiles of the block [c0, c1), query ranges outermost."""
        import math
        qp, gp = self.qset.ptr, self.gset.ptr
        cells = max(1, self.budget // 4)
        gclips = int(gp[c1] - gp[c0])
        qcap = max(math.isqrt(cells), cells // max(gclips, 1))
        qranges = _set_ranges(qp, 0, self.nq, qcap)
        qmax = max(int(qp[a1] - qp[a0]) for a0, a1 in qranges)
        granges = _set_ranges(gp, c0, c1, max(1, cells // qmax))
        return [(a0, a1, b0, b1) for a0, a1 in qranges for b0, b1 in granges]

    def block(self, c0, c1):
        n, k = c1 - c0, self.qf.shape[1]
        out = self._view(n)
        qs, gs = self.qset, self.gset
        for a0, a1, b0, b1 in self.tiles(c0, c1):
            q0, q1, g0, g1 = int(qs.ptr[a0]), int(qs.ptr[a1]), int(gs.ptr[b0]), int(gs.ptr[b1])
            M, N = q1 - q0, g1 - g0
            if self.scratch is None or self.scratch.numel() < M * N:
                self.scratch = _new((M * N,), self.qf)
            e = self.scratch[:M * N].view(M, N)
            if self.metric == 'cosine':
                gemm(qs.clips[q0:q1], gs.clips[g0:g1], e, M, N, k, epilogue=EPI_NEGDOT, math=MATH_F32)
            else:
                gemm(qs.clips[q0:q1], gs.clips[g0:g1], e, M, N, k, epilogue=EPI_EUCLID, rnorm=self.rn[q0:q1],
                     cnorm=self.cn[g0 - self.cn0:g1 - self.cn0], math=MATH_F32)
            _call('grl_setdist_block', ptr(e), N, qs.ptr.ctypes.data, ptr(qs.ptr_dev), a0, a1 - a0, gs.ptr.ctypes.data,
                  ptr(gs.ptr_dev), b0, b1 - b0, self.reduce, ptr(out[a0:, b0 - c0:]), n)
        return out


def _set_pair(qset, gset, what):
    if not (isinstance(qset, TrackletSet) and isinstance(gset, TrackletSet)):
        raise ValueError('%s: qset and gset must be TrackletSet objects (got %s, %s)'
                         % (what, type(qset).__name__, type(gset).__name__))


def set_dist(qset, gset, reduce='chamfer', metric='cosine'):
    """The materialised [nq, ng] float32 set distances between the tracklets of two ``TrackletSet``s, for small sets and
    tests.  With e the clip distances of a tracklet pair (m x p; 'cosine' = the entries of cosin_dist, 'euclidean' = of
    pairwise_distance_tensor of the clip tensors), rowmin[i] = min_j e[i][j] and colmin[j] = min_i e[i][j]:
    'min' = the closest clip pair, 'mean' = the mean of e, 'chamfer' = (mean_i rowmin[i] + mean_j colmin[j]) / 2,
    'hausdorff' = max(max_i rowmin[i], max_j colmin[j]).  min and max select exactly (-0 below +0), a NaN clip distance
    makes its cell the canonical NaN, the sums run in the fixed fp32 order of include/grl_hip.h: tests/setdist_ref.py
    gives the same bits from the clip matrix.  Only one clip x clip tile within GRL_SEARCH_BLOCK_BYTES exists at a time."""
    _set_pair(qset, gset, 'set_dist')
    _set_args(reduce, metric, 'set_dist')
    if qset.n == 0 or gset.n == 0:
        return torch.empty((qset.n, gset.n), dtype=torch.float32, device=qset.clips.device)
    return _SetBlocks(qset, gset, reduce, metric, block_cols=gset.n).block(0, gset.n).clone()


def set_search(qset, gset, k, reduce='chamfer', metric='cosine', exclude=None, block_cols=None, block_bytes=None):
    """``search`` on the set distances D = set_dist(qset, gset, reduce, metric): ``(dist [nq, k] float32, idx [nq, k]
    int64)``, bit for bit ``rank_rows(D)[:, :k]`` and D at those indices (search's tie, NaN and padding rules; ``exclude``
    is search's junk rule over the TRACKLETS' ids), without D and without the clip x clip matrix: blocks of
    ``block_cols`` gallery tracklets (default: what fits ``block_bytes`` / GRL_SEARCH_BLOCK_BYTES), each made from clip
    tiles within the same budget.  k <= 1024.  Under torch.distributed the gallery tracklets are sharded over the ranks
    and only the per-rank top-k lists are exchanged, as in ``search``."""
    _set_pair(qset, gset, 'set_search')
    _set_args(reduce, metric, 'set_search')
    k = _search_k(k, 'set_search')
    junk = _junk_ids(exclude, qset.n, gset.n, qset.clips.device)
    lo, hi, sharded = _shard(gset.n)
    blocks = _SetBlocks(qset, gset, reduce, metric, block_cols, block_bytes, lo, hi)
    return _search_blocks(blocks, qset.n, k, sharded, junk)


def set_metrics_streaming(qset, gset, q_pids, g_pids, q_camids, g_camids, reduce='chamfer', metric='cosine', max_rank=100,
                          block_cols=None, block_bytes=None):
    """``rank_metrics(rank_rows(D), ...)`` for D = set_dist(qset, gset, reduce, metric) without D: (cmc[max_rank] float32,
    mAP float) with rank_metrics_streaming's contract (first hit and #matches exact, CMC equal, mAP within 1e-12, at most
    8192 gallery tracklets per query pid) and its exchange under torch.distributed (gallery tracklets sharded)."""
    _set_pair(qset, gset, 'set_metrics_streaming')
    _set_args(reduce, metric, 'set_metrics_streaming')
    lo, hi, sharded = _shard(gset.n)
    blocks = _SetBlocks(qset, gset, reduce, metric, block_cols, block_bytes, lo, hi)
    return _metrics_from_blocks(blocks, qset.n, gset.n, q_pids, g_pids, q_camids, g_camids, max_rank, sharded)


def set_pair_roc(qset, gset, q_pids, g_pids, q_camids, g_camids, reduce='chamfer', metric='cosine', bits=ROC_BITS_DEFAULT,
                 block_cols=None, block_bytes=None):
    """``pair_roc`` on the set distances: the ``PairRoc`` of ``pair_roc_matrix(set_dist(qset, gset, reduce, metric), ...)``,
    bin for bin, without the matrix; sharded under torch.distributed as ``pair_roc`` is."""
    _set_pair(qset, gset, 'set_pair_roc')
    _set_args(reduce, metric, 'set_pair_roc')
    bits = _roc_bits(bits, 'set_pair_roc')
    lo, hi, sharded = _shard(gset.n)
    blocks = _SetBlocks(qset, gset, reduce, metric, block_cols, block_bytes, lo, hi)
    return _roc_blocks(blocks, qset.n, gset.n, q_pids, g_pids, q_camids, g_camids, bits, sharded)


# ----------------------------------------------------------------------------
# product-quantised gallery index and ADC search (pq.hip)
# ----------------------------------------------------------------------------
PQ_METRICS = {'cosine': 0, 'euclidean': 1}                            # GRL_PQ_COSINE / GRL_PQ_EUCLIDEAN of include/grl_hip.h
PQ_M_MAX = 4096                                                       # GRL_PQ_M_MAX
PQ_LUT_BYTES = int(os.environ.get('GRL_PQ_LUT_BYTES', str(1 << 30)))  # resident query tables: nq * M * ksub * 4 bytes
PQ_NQ_MAX = 262140                                                    # queries per grl_pq_scan call (its grid: 4 * 65535)


def _pq_split(d, M, what):
    """dsub = d / M, or ValueError naming M (d % M) or dsub (the sub-products go through the fp32 GEMM: K % 32 == 0)."""
    M = _int_arg(M, 1, PQ_M_MAX, what, 'M')
    if d % M:
        raise ValueError('%s: M must divide the feature size (d = %d, got M = %d)' % (what, d, M))
    if (d // M) % 32:
        raise ValueError('%s: dsub = d / M must be a multiple of 32 (d = %d, M = %d give dsub = %d)' % (what, d, M, d // M))
    return M, d // M


def _pq_rows(xf, d, what, name):
    require_device(xf, name)
    if xf.dim() != 2 or xf.shape[1] != d:
        raise ValueError('%s: %s must be [rows, d] = [rows, %d] (got %s)' % (what, name, d, tuple(xf.shape)))
    return xf.contiguous()


def _pq_codes(codes, M, what):
    if not (torch.is_tensor(codes) and codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2
            and codes.shape[1] == M):
        raise ValueError('%s: codes must be a uint8 device tensor [n, M] = [n, %d] (got %s)'
                         % (what, M, (tuple(codes.shape), codes.dtype) if torch.is_tensor(codes) else type(codes).__name__))
    return codes.contiguous()


def _pq_pack(labels, codes, n, M, ksub, what):
    """grl_pq_pack: the scan layout (uint32 [ceil(M / 4), n]) of int32 labels [M, n] (``codes`` is then written) or of
    ``codes`` (labels None), and the one-word range check: ValueError for a code outside 0..ksub-1."""
    scan = torch.empty(((M + 3) // 4, n), dtype=torch.int32, device=codes.device)
    if n:
        flag = torch.zeros(1, dtype=torch.int32, device=codes.device)
        _call('grl_pq_pack', ptr(labels), ptr(codes), ptr(scan), n, M, ksub, ptr(flag))
        if int(flag):
            raise ValueError('%s: codes must be in 0..ksub-1 = 0..%d' % (what, ksub - 1))
    return scan


class PqCodebook(object):
    """The codebooks of a product quantiser: ``codebooks`` [M, ksub, dsub] float32 on the device, subspace
    m = the feature columns [m * dsub, (m + 1) * dsub), ksub = 2**nbits centroids each (16, 32, 64, 128 or 256), dsub a
    multiple of 32; ``d`` = M * dsub.  ``metric`` ('cosine' = cosin_dist, 'euclidean' = pairwise_distance_tensor) is the
    distance the tables approximate; the codes are Euclidean-nearest centroids under both.  A caller may wrap codebooks of
    its own; ``pq_train`` fills them by k-means and then sets ``n_iter`` / ``converged`` / ``inertia`` (one entry per
    subspace; None otherwise).  ValueError names the argument that is wrong."""

    def __init__(self, codebooks, metric='cosine'):
        _cluster_metric(metric, 'PqCodebook')
        require_device(codebooks, 'codebooks')
        if codebooks.dim() != 3:
            raise ValueError('PqCodebook: codebooks must be [M, ksub, dsub] (got %s)' % (tuple(codebooks.shape),))
        M, ksub, dsub = (int(v) for v in codebooks.shape)
        if ksub not in (16, 32, 64, 128, 256):
            raise ValueError('PqCodebook: ksub must be 2**nbits with nbits in 4..8 (got ksub = %d)' % ksub)
        _pq_split(M * dsub, M, 'PqCodebook')
        self.M, self.ksub, self.dsub, self.d, self.metric = M, ksub, dsub, M * dsub, metric
        self.codebooks = codebooks.contiguous()
        self.n_iter = self.converged = self.inertia = None
        self._cn = None

    def _labels(self, xf):
        """int32 [M, n]: row m = the labels of kmeans_assign(xf[:, sub(m)].contiguous(), codebooks[m], 'euclidean')."""
        n = xf.shape[0]
        lab = torch.empty((self.M, n), dtype=torch.int32, device=xf.device)
        for m in range(self.M):
            sub = xf[:, m * self.dsub:(m + 1) * self.dsub].contiguous()
            run_key, run_val = _kmeans_top1(sub, self.codebooks[m], 'euclidean', None, None)
            lab[m] = _kmeans_relabel(run_key, run_val, self.ksub)[0]
        return lab

    def _encode(self, xf):
        xf = _pq_rows(xf, self.d, 'PqCodebook.encode', 'xf')
        n = xf.shape[0]
        codes = torch.empty((n, self.M), dtype=torch.uint8, device=xf.device)
        if n == 0:
            return codes, torch.empty(((self.M + 3) // 4, 0), dtype=torch.int32, device=xf.device)
        return codes, _pq_pack(self._labels(xf), codes, n, self.M, self.ksub, 'PqCodebook.encode')

    def encode(self, xf):
        """uint8 [n, M]: codes[i, m] = kmeans_assign(xf[:, sub(m)].contiguous(), codebooks[m], 'euclidean')[0][i], bit
        for bit -- the Euclidean-nearest centroid of the sub-row, ties to the smaller centroid index -- one byte per code
        whatever nbits is.  The clamp of pairwise_distance_tensor turns a NaN distance into 1e-12, so a NaN row ties at
        every centroid and encodes to code 0 everywhere: a consequence of that clamp, not a special case."""
        return self._encode(xf)[0]

    def decode(self, codes):
        """float32 [n, d]: decode(codes)[i, sub(m)] = codebooks[m, codes[i, m]], exact copies.  ValueError for a code
        >= ksub (one device-side check, skipped where ksub = 256 cannot be exceeded)."""
        codes = _pq_codes(codes, self.M, 'PqCodebook.decode')
        n = codes.shape[0]
        if self.ksub < 256:
            _pq_pack(None, codes, n, self.M, self.ksub, 'PqCodebook.decode')
        out = _new((n, self.d), self.codebooks)
        if n:
            _call('grl_pq_decode', ptr(self.codebooks), ptr(codes), ptr(out), n, self.M, self.ksub, self.dsub, self.d)
        return out

    def lut(self, qf):
        """The query tables [nq, M, ksub] float32.  With g = cosin_dist(qf[:, sub(m)].contiguous(), codebooks[m]) (the
        NEGDOT GEMM's bits; the GEMM reads the slice in place and writes into the table): 'cosine' lut[q, m] = g[q];
        'euclidean' lut[q, m, c] = cn[m, c] + 2 * g[q, c], cn[m] = grl_row_sqnorm of codebooks[m] (one exact multiply,
        one rounded add; the query's own norm is added by the scan)."""
        qf = _pq_rows(qf, self.d, 'PqCodebook.lut', 'qf')
        nq, M, ksub, dsub = qf.shape[0], self.M, self.ksub, self.dsub
        lut = _new((nq, M, ksub), qf)
        if nq == 0:
            return lut
        for m in range(M):
            gemm(qf[:, m * dsub:], self.codebooks[m], lut[:, m], nq, ksub, dsub, lda=self.d, ldy=M * ksub,
                 epilogue=EPI_NEGDOT, math=MATH_F32)
        if self.metric == 'euclidean':
            if self._cn is None:
                self._cn = _new((M, ksub), qf)
                _call('grl_row_sqnorm', ptr(self.codebooks), ptr(self._cn), M * ksub, dsub, dsub)
            _call('grl_pq_lut_finish', ptr(lut), ptr(self._cn), nq, M, ksub)
        return lut


def pq_train(xf, M, nbits=8, metric='cosine', max_iter=25, seed=0):
    """A ``PqCodebook`` trained on the rows of ``xf`` [n, d]: subspace m holds ``kmeans(xf[:, sub(m)].contiguous(),
    2**nbits, 'euclidean', 'random', seed + m, max_iter).centroids``, bit for bit (Euclidean k-means under both metrics, as
    is usual for product quantisation; ``metric`` only selects the tables' form).  ``n_iter``, ``converged`` and
    ``inertia`` of the result list the M runs.  Not sharded: every rank trains the full, identical codebooks.
    ValueError: a ``verify_metric``, M not dividing d, dsub = d / M not a multiple of 32, nbits outside 4..8,
    n < 2**nbits (k-means' own rule), max_iter < 1, seed < 0."""
    _cluster_metric(metric, 'pq_train')
    xf = _kmeans_rows(xf, 'pq_train')
    n, d = xf.shape
    M, dsub = _pq_split(d, M, 'pq_train')
    nbits = _int_arg(nbits, 4, 8, 'pq_train', 'nbits')
    max_iter = _kmeans_int(max_iter, 1, 'pq_train', 'max_iter')
    seed = _kmeans_int(seed, 0, 'pq_train', 'seed')
    ksub = 1 << nbits
    if n < ksub:
        raise ValueError('pq_train: xf needs at least ksub = 2**nbits = %d rows (n = %d)' % (ksub, n))
    runs = [kmeans(xf[:, m * dsub:(m + 1) * dsub].contiguous(), ksub, 'euclidean', 'random', seed + m, max_iter)
            for m in range(M)]
    book = PqCodebook(torch.stack([r.centroids for r in runs]), metric)
    book.n_iter, book.converged, book.inertia = [r.n_iter for r in runs], [r.converged for r in runs], [r.inertia for r in runs]
    return book


class PqIndex(object):
    """A gallery as product-quantiser codes: ``codebook``, ``codes`` (uint8 [n, M] on the device, the public layout),
    ``n``, and ``nbytes`` = everything the index keeps on the device: the codes, their scan-layout copy (uint32
    [ceil(M / 4), n], what grl_pq_scan reads coalesced) and the codebooks.  The constructor checks once that every code is
    below ksub (ValueError), so the scan never has to."""

    def __init__(self, codebook, codes, _scan=None):
        if not isinstance(codebook, PqCodebook):
            raise ValueError('PqIndex: codebook must be a PqCodebook (got %s)' % type(codebook).__name__)
        self.codebook, self.codes = codebook, _pq_codes(codes, codebook.M, 'PqIndex')
        self.n = int(self.codes.shape[0])
        self._scan = _pq_pack(None, self.codes, self.n, codebook.M, codebook.ksub, 'PqIndex') if _scan is None else _scan
        self.nbytes = self.codes.numel() + 4 * self._scan.numel() + 4 * codebook.codebooks.numel()


def pq_index(xf, codebook):
    """``PqIndex(codebook, codebook.encode(xf))`` with the scan layout written by the same launch as the codes."""
    if not isinstance(codebook, PqCodebook):
        raise ValueError('pq_index: codebook must be a PqCodebook (got %s)' % type(codebook).__name__)
    codes, scan = codebook._encode(xf)
    return PqIndex(codebook, codes, scan)


class _PqBlocks(_BlockSource):
    """Column blocks of the ADC distance matrix of ``qf`` against the code rows of ``index``: a ``_BlockSource`` (widths
    chosen as ``_ColumnBlocks`` does).  The constructor makes the tables of all its queries (``codebook.lut``) and, for 'euclidean', their
    grl_row_sqnorm; a block is one grl_pq_scan over the code rows [c0, c1).  An entry's bits depend on its codes and its
    query's table alone (include/grl_hip.h), so a block holds the full matrix's bits whatever its width."""

    def __init__(self, qf, index, block_cols=None, block_bytes=None):
        _check_index(index, PqIndex, '_PqBlocks')
        book = index.codebook
        self.qf = _pq_rows(qf, book.d, '_PqBlocks', 'qf')
        self.index, self.nq, self.ng = index, self.qf.shape[0], index.n
        self._cut(0, index.n, block_cols, block_bytes)
        self.lut = self.rn = None
        if self.spans and self.nq:
            self.lut = book.lut(self.qf)
            if book.metric == 'euclidean':
                self.rn = _new((self.nq,), self.qf)
                _call('grl_row_sqnorm', ptr(self.qf), ptr(self.rn), self.nq, book.d, book.d)

    def block(self, c0, c1):
        n, book = c1 - c0, self.index.codebook
        out = self._view(n)
        scan = self.index._scan
        if n != self.ng:                                   # the kernel's row stride is its column count
            scan = scan[:, c0:c1].contiguous()
        _call('grl_pq_scan', ptr(self.lut), ptr(scan), ptr(out), self.nq, n, book.M, book.ksub, n,
              PQ_METRICS[book.metric], ptr(self.rn))
        return out


def pq_dist(qf, index, block_cols=None, block_bytes=None):
    """The materialised [nq, n] float32 ADC distances of ``qf`` against ``index``, for small cases and tests: per pair the
    sum S of the M table entries its codes select, in the fixed fp32 order of include/grl_hip.h (four partials, adds only);
    'cosine': S; 'euclidean': sqrt(max(|q|^2 + S, 1e-12)), a NaN argument giving 1e-12 as in pairwise_distance_tensor.
    tests/pq_ref.py gives the same bits from the tables.  The same bits for every ``block_cols``."""
    _check_index(index, PqIndex, 'pq_dist')
    blocks = _PqBlocks(qf, index, index.n if block_cols is None and block_bytes is None else block_cols, block_bytes)
    return _dist_from_blocks(blocks, index.n)


def pq_search(qf, index, k, exclude=None, block_cols=None, block_bytes=None):
    """``search`` on the ADC distances D = pq_dist(qf, index): ``(dist [nq, k] float32, idx [nq, k] int64)``, bit for bit
    ``rank_rows(D)[:, :k]`` and D at those indices, without D: blocks of code rows through grl_pq_scan, ranked by
    search's running top-k.  Identical code rows give identical distances, so ties are the rule here: they go to the
    smaller gallery index.  ``exclude`` is search's junk rule; padding is index -1, distance +inf; k <= 1024.  The tables
    of the queries are resident (nq * M * ksub * 4 bytes); beyond GRL_PQ_LUT_BYTES (1 GiB) the queries are served in row
    blocks, whose results are independent and concatenated.  Not sharded: every rank computes the full result."""
    _check_index(index, PqIndex, 'pq_search')
    k, book = _search_k(k, 'pq_search'), index.codebook
    qf = _pq_rows(qf, book.d, 'pq_search', 'qf')
    junk = _junk_ids(exclude, qf.shape[0], index.n, qf.device)
    rows = max(1, PQ_LUT_BYTES // (4 * book.M * book.ksub))          # queries whose tables fit (at least one)
    return _search_by_query_rows(lambda q: _PqBlocks(q, index, block_cols, block_bytes), qf, rows, k, junk)


def pq_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids, max_rank=100, block_cols=None, block_bytes=None):
    """``rank_metrics(rank_rows(D), ...)`` for D = pq_dist(qf, index) without D: (cmc[max_rank] float32, mAP float) with
    rank_metrics_streaming's contract.  The tables of ALL queries must fit GRL_PQ_LUT_BYTES: ValueError otherwise, naming
    the bytes (the two passes walk every query's matches together).  Not sharded."""
    _check_index(index, PqIndex, 'pq_metrics_streaming')
    book = index.codebook
    qf = _pq_rows(qf, book.d, 'pq_metrics_streaming', 'qf')
    need = 4 * qf.shape[0] * book.M * book.ksub
    if need > PQ_LUT_BYTES:
        raise ValueError('pq_metrics_streaming: the query tables take %d bytes (nq * M * ksub * 4 = %d * %d * %d * 4), above '
                         'GRL_PQ_LUT_BYTES = %d' % (need, qf.shape[0], book.M, book.ksub, PQ_LUT_BYTES))
    blocks = _PqBlocks(qf, index, block_cols, block_bytes)
    return _metrics_from_blocks(blocks, blocks.nq, index.n, q_pids, g_pids, q_camids, g_camids, max_rank, False)


def topk_recall(approx_idx, exact_idx, ks):
    """Host helper: for each k of ``ks``, the mean over the queries of |approx[:k] & exact[:k]| / (number of valid entries
    of exact[:k]), as a list of floats.  The index lists are ``search``'s ([nq, L] tensors or arrays, -1 = padding, which
    matches nothing); a query whose exact[:k] is all padding is left out of the mean (nan when none is left)."""
    import numpy as np
    a = np.asarray(approx_idx.cpu() if torch.is_tensor(approx_idx) else approx_idx).astype(np.int64)
    e = np.asarray(exact_idx.cpu() if torch.is_tensor(exact_idx) else exact_idx).astype(np.int64)
    if a.ndim != 2 or e.ndim != 2 or a.shape[0] != e.shape[0]:
        raise ValueError('topk_recall: approx_idx and exact_idx must be [nq, L] lists of the same queries (got %s, %s)'
                         % (a.shape, e.shape))
    out = []
    for k in ks:
        k = _int_arg(k, 1, _INT_MAX, 'topk_recall', 'k')
        part = []
        for ra, re_ in zip(a[:, :k], e[:, :k]):
            valid = re_[re_ >= 0]
            if valid.size:
                part.append(np.intersect1d(ra[ra >= 0], valid).size / float(valid.size))
        out.append(float(np.mean(part)) if part else float('nan'))
    return out


# ----------------------------------------------------------------------------
# IVF-PQ index: inverted lists over residual product-quantiser codes (ivf.hip)
# ----------------------------------------------------------------------------
IVF_NLIST_MAX, IVF_NPROBE_MAX = 65536, 1024                           # GRL_IVF_NLIST_MAX / GRL_IVF_NPROBE_MAX


class IvfPqCodebook(object):
    """The quantisers of an IVFADC index: ``coarse`` [nlist, d] float32 on the device, the centroids of the
    inverted lists (1 <= nlist <= 65536), and ``pq``, a ``PqCodebook`` over the RESIDUALS row - coarse[list] whose own
    metric is 'cosine', so that its tables are the plain NEGDOT tables lut[q, m, c] = -q_m . R[m][c] under both index
    metrics.  ``metric`` ('cosine' = cosin_dist, 'euclidean' = pairwise_distance_tensor) is the distance the index
    approximates.  A caller may wrap tensors of its own; ``ivf_train`` fills them by k-means and then sets
    ``coarse_n_iter`` / ``coarse_converged`` / ``coarse_inertia`` (None otherwise; the product quantiser's are on ``pq``).
    ValueError names the argument that is wrong."""

    def __init__(self, coarse, pq, metric='cosine'):
        _cluster_metric(metric, 'IvfPqCodebook')
        require_device(coarse, 'coarse')
        if coarse.dim() != 2:
            raise ValueError('IvfPqCodebook: coarse must be [nlist, d] (got %s)' % (tuple(coarse.shape),))
        nlist, d = (int(v) for v in coarse.shape)
        if not 1 <= nlist <= IVF_NLIST_MAX:
            raise ValueError('IvfPqCodebook: coarse must hold nlist in 1..%d centroids (got nlist = %d)' % (IVF_NLIST_MAX, nlist))
        if not isinstance(pq, PqCodebook):
            raise ValueError('IvfPqCodebook: pq must be a PqCodebook (got %s)' % type(pq).__name__)
        if pq.metric != 'cosine':
            raise ValueError("IvfPqCodebook: pq must be a PqCodebook whose metric is 'cosine' (the residual tables are the "
                             'NEGDOT tables under both index metrics; got %r)' % (pq.metric,))
        if pq.d != d:
            raise ValueError('IvfPqCodebook: pq.d must equal the feature size of coarse (pq.d = %d, d = %d)' % (pq.d, d))
        self.coarse, self.pq, self.metric, self.nlist, self.d = coarse.contiguous(), pq, metric, nlist, d
        self.coarse_n_iter = self.coarse_converged = self.coarse_inertia = None


def _ivf_book(book, what):
    if not isinstance(book, IvfPqCodebook):
        raise ValueError('%s: book must be an IvfPqCodebook (got %s)' % (what, type(book).__name__))


def _ivf_residual(xf, labels32, coarse, out):
    rows, d = xf.shape
    if rows:
        _call('grl_ivf_residual', ptr(xf), xf.stride(0), ptr(labels32), ptr(coarse), coarse.shape[0], ptr(out), d, rows, d)
    return out


def ivf_train(xf, nlist, M, nbits=8, metric='cosine', max_iter=25, seed=0):
    """An ``IvfPqCodebook`` trained on the rows of ``xf`` [n, d], in three steps, bit for bit:
      coarse = kmeans(xf, nlist, 'euclidean', 'random', seed, max_iter).centroids
      lab    = kmeans_assign(xf, coarse, 'euclidean')[0]
      pq     = pq_train(r, M, nbits, 'cosine', max_iter, seed + 1),  r[i][c] = xf[i][c] - coarse[lab_i][c] (one rounded
               subtraction, grl_ivf_residual)
    Both quantisers are Euclidean under both metrics; ``metric`` only selects the distance the index
    approximates.  The residual copy r (n * d * 4 bytes) lives for the call: train on a subsample.  Not sharded.
    ValueError: a ``verify_metric``, pq_train's rules on M, dsub and nbits, nlist outside 1..65536, max_iter < 1,
    seed < 0, n < max(nlist, 2**nbits)."""
    _cluster_metric(metric, 'ivf_train')
    xf = _kmeans_rows(xf, 'ivf_train')
    n, d = xf.shape
    M, dsub = _pq_split(d, M, 'ivf_train')
    nbits = _int_arg(nbits, 4, 8, 'ivf_train', 'nbits')
    nlist = _int_arg(nlist, 1, IVF_NLIST_MAX, 'ivf_train', 'nlist')
    max_iter = _kmeans_int(max_iter, 1, 'ivf_train', 'max_iter')
    seed = _kmeans_int(seed, 0, 'ivf_train', 'seed')
    if n < max(nlist, 1 << nbits):
        raise ValueError('ivf_train: xf needs at least max(nlist, 2**nbits) = %d rows (n = %d)' % (max(nlist, 1 << nbits), n))
    run = kmeans(xf, nlist, 'euclidean', 'random', seed, max_iter)
    lab = kmeans_assign(xf, run.centroids, 'euclidean')[0]
    res = _ivf_residual(xf, lab.to(torch.int32), run.centroids, _new((n, d), xf))
    pq = pq_train(res, M, nbits, 'cosine', max_iter, seed + 1)
    del res
    book = IvfPqCodebook(run.centroids, pq, metric)
    book.coarse_n_iter, book.coarse_converged, book.coarse_inertia = run.n_iter, run.converged, run.inertia
    return book


class IvfPqIndex(object):
    """A gallery as inverted lists of residual product-quantiser codes.  ``IvfPqIndex(book, labels,
    codes)`` builds it from caller-supplied ``labels`` (an integer device tensor [n], the list of every gallery row) and
    ``codes`` (uint8 device [n, M], the codes of the residuals, gallery order); one device-side range check each: labels
    in 0..nlist-1, codes < ksub (ValueError).  Empty lists are legal; n < 2**31.  It keeps

      list_ptr  int64 [nlist + 1]   list l = the list positions list_ptr[l] .. list_ptr[l + 1]
      ids       int32 [n]           the gallery index at every list position, ASCENDING inside a list (grl_kmeans_members)
      codes     uint8 [n, M]        the public layout, gallery order
      xn        float32 [n]         'euclidean' only: grl_row_sqnorm of the reconstructed row, list order
      n, nbytes                     nbytes counts everything resident: the above, the scan layout (uint32 [ceil(M / 4), n],
                                    list order), the labels (int32 [n]), coarse and the codebooks

    ``labels()`` returns the list of every gallery row (int64), ``reconstruct(rows)`` the approximation
    x^[i][sub(m)] = coarse[lab_i][sub(m)] + R[m][code[i, m]] (one rounded add per element) of the given gallery indices."""

    def __init__(self, book, labels, codes):
        self._build(book, labels, codes, True)

    @classmethod
    def _from_assigned(cls, book, labels, codes):
        """the index of labels that kmeans_assign made: they are inside 0..nlist-1 already, so the label check is skipped"""
        index = cls.__new__(cls)
        index._build(book, labels, codes, False)
        return index

    def _build(self, book, labels, codes, check_labels):
        _ivf_book(book, 'IvfPqIndex')
        pq = book.pq
        codes = _pq_codes(codes, pq.M, 'IvfPqIndex')
        n = int(codes.shape[0])
        if not (torch.is_tensor(labels) and labels.is_cuda and labels.dim() == 1 and labels.numel() == n
                and not labels.dtype.is_floating_point and not labels.dtype.is_complex and labels.dtype != torch.bool):
            raise ValueError('IvfPqIndex: labels must be an integer device tensor with one entry per row of codes (%d)' % n)
        if n >= 2 ** 31:
            raise ValueError('IvfPqIndex: n must be below 2**31 (got %d)' % n)
        dev, nlist = codes.device, book.nlist
        lab32 = labels.to(torch.int64).clamp(min=-1, max=IVF_NLIST_MAX).to(torch.int32).contiguous()
        if n and check_labels:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            _call('grl_ivf_check_labels', ptr(lab32), n, nlist, ptr(flag))
            if int(flag):
                raise ValueError('IvfPqIndex: labels must be in 0..nlist-1 = 0..%d' % (nlist - 1))
        counts = torch.zeros(nlist, dtype=torch.int32, device=dev)
        self.list_ptr = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
        self.ids = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            _call('grl_kmeans_label_counts', ptr(lab32), n, nlist, ptr(counts))
            _call('grl_rrs_scan', ptr(counts), nlist, ptr(self.list_ptr))
            cursor = torch.zeros(nlist, dtype=torch.int32, device=dev)
            tmp = torch.empty(n, dtype=torch.int32, device=dev)
            _call('grl_kmeans_members', ptr(lab32), n, nlist, ptr(self.list_ptr), ptr(cursor), ptr(tmp), ptr(self.ids))
        order = self.ids.to(torch.int64)
        self._scan = _pq_pack(None, codes[order].contiguous(), n, pq.M, pq.ksub, 'IvfPqIndex')   # (the codes' range check)
        self.book, self.codes, self.n, self._labels = book, codes, n, lab32
        self._lens = counts.to(torch.int64)
        lens = sorted((int(v) for v in counts.cpu().tolist()), reverse=True)     # the build's one read-back of the lengths
        self.list_len_min, self.list_len_max = (lens[-1], lens[0])
        self._longest = [0]                                # _longest[c] = the sum of the c longest lists: a chunk's width bound
        for v in lens[:IVF_NPROBE_MAX]:
            self._longest.append(self._longest[-1] + v)
        self.xn = None
        if book.metric == 'euclidean':
            self.xn = _new((n,), book.coarse)
            rows = max(1, SEARCH_BLOCK_BYTES // (4 * book.d))
            for b0 in range(0, n, rows):
                pos = order[b0:b0 + rows]
                x = self._reconstruct(lab32[pos].contiguous(), codes[pos].contiguous())
                _call('grl_row_sqnorm', ptr(x), ptr(self.xn[b0:]), x.shape[0], book.d, book.d)
        self.nbytes = (8 * (nlist + 1) + 4 * n + codes.numel() + 4 * self._scan.numel() + 4 * n
                       + (4 * n if self.xn is not None else 0) + 4 * book.coarse.numel() + 4 * pq.codebooks.numel())

    def _reconstruct(self, lab32, codes):
        book, pq = self.book, self.book.pq
        rows = codes.shape[0]
        out = _new((rows, book.d), book.coarse)
        if rows:
            _call('grl_ivf_reconstruct', ptr(book.coarse), ptr(pq.codebooks), ptr(lab32), ptr(codes), ptr(out), rows, book.nlist,
                  pq.M, pq.ksub, pq.dsub, book.d)
        return out

    def labels(self):
        return self._labels.to(torch.int64)

    def reconstruct(self, rows):
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 1 and not rows.dtype.is_floating_point
                and not rows.dtype.is_complex and rows.dtype != torch.bool):
            raise ValueError('IvfPqIndex.reconstruct: rows must be a 1-d integer device tensor of gallery indices')
        rows = rows.to(torch.int64)
        if rows.numel() and bool(((rows < 0) | (rows >= self.n)).any()):
            raise ValueError('IvfPqIndex.reconstruct: rows must be in 0..n-1 = 0..%d' % (self.n - 1))
        return self._reconstruct(self._labels[rows].contiguous(), self.codes[rows].contiguous())


def ivf_index(xf, book):
    """The ``IvfPqIndex`` of the rows of ``xf`` [n, d]: labels = kmeans_assign(xf, book.coarse, 'euclidean')[0] (a NaN row
    lands in list 0 with code 0 everywhere: pairwise_distance_tensor's clamp, not a special case), the residuals encoded
    by ``book.pq`` in row blocks whose residual buffer fits GRL_SEARCH_BLOCK_BYTES -- an n x d residual is never built."""
    _ivf_book(book, 'ivf_index')
    xf = _pq_rows(xf, book.d, 'ivf_index', 'xf')
    n, d, pq = xf.shape[0], book.d, book.pq
    if n >= 2 ** 31:
        raise ValueError('ivf_index: n must be below 2**31 (got %d)' % n)
    codes = torch.empty((n, pq.M), dtype=torch.uint8, device=xf.device)
    if n == 0:
        return IvfPqIndex._from_assigned(book, torch.empty(0, dtype=torch.int64, device=xf.device), codes)
    lab = kmeans_assign(xf, book.coarse, 'euclidean')[0]
    lab32 = lab.to(torch.int32)
    rows = max(1, min(n, SEARCH_BLOCK_BYTES // (4 * d)))
    res = _new((rows, d), xf)
    for b0 in range(0, n, rows):
        b1 = min(b0 + rows, n)
        codes[b0:b1] = pq._encode(_ivf_residual(xf[b0:b1], lab32[b0:b1], book.coarse, res[:b1 - b0]))[0]
    return IvfPqIndex._from_assigned(book, lab, codes)


def _ivf_args(qf, index, nprobe, what):
    _check_index(index, IvfPqIndex, what)
    hi = min(index.book.nlist, IVF_NPROBE_MAX)
    nprobe = _int_arg(nprobe, 1, hi, what, 'nprobe')
    return _pq_rows(qf, index.book.d, what, 'qf'), nprobe


def _ivf_probe(qf, book, nprobe):
    """(probe int64 [nq, nprobe], g0 float32 [nq, nprobe]): the index list of search(qf, coarse, nprobe, metric), unsharded
    (every rank probes alike), and G0 = cosin_dist(qf, coarse) [nq, nlist] gathered there."""
    probe = _ivf_probe_lists(qf, book, nprobe)
    return probe, cosin_dist(qf, book.coarse).gather(1, probe).contiguous()


def _ivf_probe_lists(qf, book, nprobe):
    return _search_blocks(_ColumnBlocks(qf, book.coarse, book.metric), qf.shape[0], nprobe, False)[1]


class _IvfQueries(object):
    """What a block of query rows needs for its scans: the residual tables (``book.pq.lut``), the probes = the index
    list of search(qf, coarse, nprobe, metric) (unsharded: every rank probes alike), G0 = cosin_dist(qf, coarse)
    gathered at the probes, the probed lists' lengths and, for 'euclidean', grl_row_sqnorm of the queries.
    ``chunk(j0, j1, width)`` is one grl_ivf_scan over the probe ranks [j0, j1): (dist [nq, width], cidx [nq, width])."""

    def __init__(self, qf, index, nprobe):
        book = index.book
        self.index, self.qf, self.nq = index, qf, qf.shape[0]
        nq = self.nq
        self.lut = book.pq.lut(qf)
        probe, self.g0 = _ivf_probe(qf, book, nprobe)
        self.plen = index._lens[probe]
        self.probe = probe.to(torch.int32).contiguous()
        self.rn = None
        if book.metric == 'euclidean':
            self.rn = _new((nq,), qf)
            _call('grl_row_sqnorm', ptr(qf), ptr(self.rn), nq, book.d, book.d)
        self.buf = self.cbuf = None

    def chunk(self, j0, j1, width):
        index, nq, c = self.index, self.nq, j1 - j0
        book, pq = index.book, index.book.pq
        if self.buf is None or self.buf.numel() < nq * width:
            self.buf = _new((nq * width,), self.qf)
            self.cbuf = torch.empty(nq * width, dtype=torch.int32, device=self.qf.device)
        out, cidx = self.buf[:nq * width].view(nq, width), self.cbuf[:nq * width].view(nq, width)
        off = torch.zeros((nq, c + 1), dtype=torch.int32, device=self.qf.device)
        off[:, 1:] = self.plen[:, j0:j1].cumsum(1)
        probe, g0 = self.probe, self.g0
        if c != probe.shape[1]:
            probe, g0 = probe[:, j0:j1].contiguous(), g0[:, j0:j1].contiguous()
        _call('grl_ivf_scan', ptr(self.lut), ptr(index._scan), ptr(index.ids), ptr(index.list_ptr), ptr(probe), ptr(g0), c, c,
              ptr(off), ptr(index.xn), ptr(self.rn), ptr(out), ptr(cidx), width, width, nq, index.n, book.nlist, pq.M, pq.ksub,
              PQ_METRICS[book.metric])
        return out, cidx


def _ivf_plan(index, nq, nprobe, block_bytes):
    """(query rows per block, probes per chunk): a chunk row is at most the sum of the chunk's longest lists wide (known
    from the build, no read-back), and the distance block plus the cidx block (8 bytes per entry) fit the budget; a chunk
    holds at least one probe, and where one probe already exceeds the budget the queries go in row blocks.  The tables
    obey GRL_PQ_LUT_BYTES and a launch serves at most 65535 queries."""
    pq = index.book.pq
    budget = _block_budget(block_bytes)
    rows = max(1, min(65535, PQ_LUT_BYTES // (4 * pq.M * pq.ksub), max(nq, 1)))
    one = max(index._longest[1], 1)
    if 8 * rows * one > budget:
        rows = max(1, budget // (8 * one))
    per = 1
    while per < nprobe and 8 * rows * max(index._longest[per + 1], 1) <= budget:
        per += 1
    return rows, per


def ivf_search(qf, index, k, nprobe, exclude=None, block_bytes=None):
    """Each query's ``k`` nearest among the rows of the ``nprobe`` inverted lists nearest to it: ``(dist [nq, k] float32,
    idx [nq, k] int64)``.  The probes are the index list of search(qf, coarse, nprobe, metric) (ties to the smaller list);
    a candidate's distance is the normative one of include/grl_hip.h (g0 + the ADC sum over its residual codes; for
    'euclidean' the reconstructed row's and the query's norms added and the clamped square root); the result is the
    first k candidates in grl_row_argsort's order (canonical NaN, -0 == +0, ties to the smaller GALLERY index) with those
    distances.  ``exclude`` is search's junk rule, applied through grl_topk_block_filtered and the scan's cidx: no mask is
    built.  Fewer than k candidates leave padding: index -1, distance +inf.  k <= 1024; 1 <= nprobe <= min(nlist, 1024).
    The candidates are served in chunks of probe ranks sized by ``block_bytes`` (default GRL_SEARCH_BLOCK_BYTES), the
    queries in row blocks where one probe exceeds it or the tables exceed GRL_PQ_LUT_BYTES: the same bits for every
    chunking.  Not sharded: every rank computes the full result."""
    _check_index(index, IvfPqIndex, 'ivf_search')
    k = _search_k(k, 'ivf_search')
    qf, nprobe = _ivf_args(qf, index, nprobe, 'ivf_search')
    nq, dev = qf.shape[0], qf.device
    junk = _junk_ids(exclude, nq, index.n, dev)
    top = _TopK(nq, k, dev)
    if nq and index.n:
        rows, per = _ivf_plan(index, nq, nprobe, block_bytes)
        for q0 in range(0, nq, rows):
            q1 = min(q0 + rows, nq)
            qs = _IvfQueries(qf[q0:q1], index, nprobe)
            for j0 in range(0, nprobe, per):
                j1 = min(j0 + per, nprobe)
                width = min(index._longest[j1 - j0], index.n)
                if width == 0:
                    continue
                d, cidx = qs.chunk(j0, j1, width)
                top.push(d, width, width, 0, cidx, width, junk, (q0, q1))
    return top.result()


def ivf_dist(qf, index, nprobe):
    """The materialised form of ``ivf_search``'s candidates, for small cases and tests: ``(D [nq, n] float32, cand [nq, n]
    bool)`` in gallery order; cand[q, i] = row i is in one of q's probed lists, D[q, i] its normative distance (defined
    where cand is set, 0 elsewhere)."""
    qf, nprobe = _ivf_args(qf, index, nprobe, 'ivf_dist')
    nq, n = qf.shape[0], index.n
    D = torch.zeros((nq, n), dtype=torch.float32, device=qf.device)
    cand = torch.zeros((nq, n), dtype=torch.bool, device=qf.device)
    width = min(index._longest[nprobe], n)
    if nq and width:
        for q0 in range(0, nq, 65535):
            qs = _IvfQueries(qf[q0:q0 + 65535], index, nprobe)
            d, cidx = qs.chunk(0, nprobe, width)
            live = cidx >= 0
            row = (torch.arange(qs.nq, device=qf.device) + q0).view(-1, 1).expand_as(cidx)[live]
            col = cidx[live].to(torch.int64)
            D[row, col] = d[live]
            cand[row, col] = True
    return D, cand


def ivf_probe_stats(qf, index, nprobe):
    """int64 [nq] on the device: the number of candidates (the summed lengths of the probed lists) of every query; their
    sum / (nq * n) is the scanned fraction."""
    qf, nprobe = _ivf_args(qf, index, nprobe, 'ivf_probe_stats')
    nq = qf.shape[0]
    if nq == 0:
        return torch.zeros(0, dtype=torch.int64, device=qf.device)
    return index._lens[_ivf_probe_lists(qf, index.book, nprobe)].sum(1)


# ----------------------------------------------------------------------------
# exact refinement of a shortlist from a feature store (refine.hip)
# ----------------------------------------------------------------------------
REFINE_D_MAX = 16384                                                  # GRL_REFINE_D_MAX
REFINE_TYPES = {'f32': 0, 'bf16': 1}                                  # GRL_REFINE_F32 / GRL_REFINE_BF16 of include/grl_hip.h


def _refine_d(d, what, name):
    if d % 4 or not 1 <= d <= REFINE_D_MAX:
        raise ValueError('%s: %s must have d columns with d a multiple of 4 in 1..%d (got d = %d)' % (what, name, REFINE_D_MAX, d))


class RefineStore(object):
    """The feature rows a shortlist is refined against: ``RefineStore(xf, dtype='f32' | 'bf16')`` of the
    contiguous float32 device tensor ``xf`` [n, d], d a multiple of 4 in 1..16384, n < 2**31.  'f32' wraps ``xf`` without
    a copy; 'bf16' makes an [n, d] copy with grl_refine_pack_bf16 (round to nearest even, every NaN 0x7fc0, infinities
    and zeros preserved): half the bytes.  A row's VALUE is the float32 widening of what is stored, and every distance of
    ``refine_dist`` is defined on the values.  ``n``, ``d``, ``dtype``, ``nbytes``; ``rows(ids)`` returns the values of
    the given rows as float32.  ValueError names the argument that is wrong."""

    def __init__(self, xf, dtype='f32'):
        if dtype not in REFINE_TYPES:
            raise ValueError("RefineStore: dtype must be 'f32' or 'bf16' (got %r)" % (dtype,))
        if not torch.is_tensor(xf) or xf.dim() != 2:
            raise ValueError('RefineStore: xf must be a [n, d] tensor (got %s)'
                             % (tuple(xf.shape) if torch.is_tensor(xf) else type(xf).__name__,))
        n, d = (int(v) for v in xf.shape)
        _refine_d(d, 'RefineStore', 'xf')
        if n >= 2 ** 31:
            raise ValueError('RefineStore: xf must have fewer than 2**31 rows (got %d)' % n)
        require_device(xf, 'xf')
        if not xf.is_contiguous():
            raise ValueError('RefineStore: xf must be contiguous (got strides %s)' % (tuple(xf.stride()),))
        self.n, self.d, self.dtype = n, d, dtype
        if dtype == 'f32':
            self.data = xf
        else:
            self.data = torch.empty((n, d), dtype=torch.bfloat16, device=xf.device)
            if n:
                _call('grl_refine_pack_bf16', ptr(xf), ptr(self.data), n * d)
        self.nbytes = n * d * (4 if dtype == 'f32' else 2)

    def rows(self, ids):
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.dim() == 1 and not ids.dtype.is_floating_point
                and not ids.dtype.is_complex and ids.dtype != torch.bool):
            raise ValueError('RefineStore.rows: ids must be a 1-d integer device tensor of row indices')
        ids = ids.to(torch.int64)
        if ids.numel() and bool(((ids < 0) | (ids >= self.n)).any()):
            raise ValueError('RefineStore.rows: ids must be in 0..n-1 = 0..%d' % (self.n - 1))
        return self.data[ids].to(torch.float32)


def _refine_args(qf, store, cand, metric, what):
    _cluster_metric(metric, what)
    if not isinstance(store, RefineStore):
        raise ValueError('%s: store must be a RefineStore (got %s)' % (what, type(store).__name__))
    if not torch.is_tensor(qf) or qf.dim() != 2 or qf.shape[1] != store.d:
        raise ValueError('%s: qf must be [rows, d] = [rows, %d] (got %s)'
                         % (what, store.d, tuple(qf.shape) if torch.is_tensor(qf) else type(qf).__name__))
    if not (torch.is_tensor(cand) and cand.dim() == 2 and cand.dtype == torch.int64 and cand.shape[0] == qf.shape[0]):
        raise ValueError('%s: cand must be an int64 device tensor [nq, L] = [%d, L] (got %s)'
                         % (what, qf.shape[0], (tuple(cand.shape), cand.dtype) if torch.is_tensor(cand) else type(cand).__name__))
    require_device(qf, 'qf')
    if not cand.is_cuda:
        raise ValueError('%s: cand must be an int64 device tensor [nq, L] (got a tensor on %s)' % (what, cand.device))
    return qf.contiguous(), cand.contiguous()


def _refine_scan(qf, store, cand, metric, out, cidx):
    """one grl_refine_scan: out / cidx [rows, L] of the (at most 65535) query rows ``qf`` and their lists ``cand``"""
    rows, L = cand.shape
    _call('grl_refine_scan', ptr(qf), store.d, ptr(store.data), store.d, REFINE_TYPES[store.dtype], ptr(cand), L, ptr(out),
          ptr(cidx), L, rows, L, store.n, store.d, PQ_METRICS[metric])


def refine_dist(qf, store, cand, metric='cosine'):
    """The [nq, L] float32 distance block of the index lists ``cand`` (int64 [nq, L] on the device: ``search``'s,
    ``pq_search``'s or ``ivf_search``'s index lists as they come) against the rows of ``store``, for tests and small
    cases: entry (q, j) is the normative pair distance of include/grl_hip.h between qf[q] and the value of store row
    cand[q, j] -- 'cosine' the negated dot product, 'euclidean' sqrt(max(sum (q - x)^2, 1e-12)) with the difference taken
    first -- in a fixed fp32 order (no fma, no atomics): tests/refine_ref.py gives the same bits.  An entry < 0 or >= n is
    padding: never dereferenced, +inf."""
    qf, cand = _refine_args(qf, store, cand, metric, 'refine_dist')
    nq, L = cand.shape
    out = torch.full((nq, L), float('inf'), dtype=torch.float32, device=qf.device)
    if nq and L and store.n:
        cidx = torch.empty((min(nq, 65535), L), dtype=torch.int32, device=qf.device)
        for q0 in range(0, nq, 65535):
            q1 = min(q0 + 65535, nq)
            _refine_scan(qf[q0:q1], store, cand[q0:q1], metric, out[q0:q1], cidx[:q1 - q0])
    return out


def refine_lists(qf, store, cand, k, metric='cosine', block_bytes=None):
    """The candidates ``cand`` (int64 [nq, L] on the device, any L; an entry < 0 or >= n is padding, a repeated id is a
    candidate twice) of every query re-sorted by their exact distances to the rows of ``store``: ``(dist [nq, k] float32,
    idx [nq, k] int64)``, the first k of each row's candidates in grl_row_argsort's order (canonical NaN, -0 == +0, ties to
    the smaller gallery index) with the normative distances of ``refine_dist``; padding is index -1, distance +inf.
    1 <= k <= 1024.  The distance block and the id block (8 bytes per pair) are served in query row blocks that fit
    ``block_bytes`` (default GRL_SEARCH_BLOCK_BYTES), each ranked by grl_topk_block with the id block as its cidx: the
    same bits for every blocking.  A ``verify_metric`` is refused.  Not sharded: every rank computes the full result."""
    k = _int_arg(k, 1, SEARCH_K_MAX, 'refine_lists', 'k')
    qf, cand = _refine_args(qf, store, cand, metric, 'refine_lists')
    nq, L = cand.shape
    dev = qf.device
    top = _TopK(nq, k, dev)
    if nq and L and store.n:
        rows = max(1, min(65535, nq, _block_budget(block_bytes) // (8 * L)))
        d = _new((rows, L), qf)
        cidx = torch.empty((rows, L), dtype=torch.int32, device=dev)
        for q0 in range(0, nq, rows):
            q1 = min(q0 + rows, nq)
            _refine_scan(qf[q0:q1], store, cand[q0:q1], metric, d, cidx)
            top.push(d, L, L, 0, cidx, L, rows=(q0, q1))
    return top.result()


def refine_search(qf, index, store, k, R, nprobe=None, exclude=None, block_bytes=None):
    """Two-stage search: a shortlist of ``R`` candidates per query from the codes of ``index`` (a ``PqIndex``: pq_search;
    an ``IvfPqIndex``: ivf_search with ``nprobe``, which is required there and refused for the flat index), re-sorted by
    the exact distances to the rows of ``store`` -- exactly ``refine_lists(qf, store, S(qf, index, R, ..., exclude=exclude)[1],
    k, index metric)``.  The junk rule ``exclude`` is applied in the first stage and nowhere else.  k <= R <= 1024;
    store.n and store.d must be the index's.  ValueError names the argument that is wrong."""
    if isinstance(index, PqIndex):
        flat, metric, d = True, index.codebook.metric, index.codebook.d
        if nprobe is not None:
            raise ValueError('refine_search: nprobe is for an IvfPqIndex; a PqIndex scans every row (got nprobe = %r)' % (nprobe,))
    elif isinstance(index, IvfPqIndex):
        flat, metric, d = False, index.book.metric, index.book.d
        if nprobe is None:
            raise ValueError('refine_search: nprobe is required for an IvfPqIndex')
    else:
        raise ValueError('refine_search: index must be a PqIndex or an IvfPqIndex (got %s)' % type(index).__name__)
    def shortlist(R):
        if flat:
            return pq_search(qf, index, R, exclude=exclude, block_bytes=block_bytes)
        return ivf_search(qf, index, R, nprobe, exclude=exclude, block_bytes=block_bytes)
    return _two_stage('refine_search', qf, index, d, metric, store, k, R, shortlist, block_bytes)


# ----------------------------------------------------------------------------
# kNN-graph gallery index with beam search on the device (nng.hip)
# ----------------------------------------------------------------------------
NNG_K_MAX, NNG_D_MAX = 128, 64                                        # GRL_NNG_* of include/grl_hip.h
NNG_L_MIN, NNG_L_MAX, NNG_W_MAX, NNG_WD_MAX = 8, 512, 8, 256
NNG_LDS_MAX = 65536
NNG_QUERY_BLOCK = int(os.environ.get('GRL_NNG_QUERY_BLOCK', '65535'))  # queries per grl_nng_search call (1..65535)


def _nng_store(x, dtype, what, name):
    """``x`` as a RefineStore: a store as it is, a float32 device tensor [n, d] wrapped (``dtype``)"""
    if isinstance(x, RefineStore):
        return x, False
    if not torch.is_tensor(x):
        raise ValueError('%s: %s must be a RefineStore or a [n, d] float32 device tensor (got %s)' % (what, name, type(x).__name__))
    return RefineStore(x.contiguous() if x.dim() == 2 else x, dtype), dtype != 'f32'


def nng_knn(store_or_xf, K, metric='cosine', block_bytes=None):
    """int64 [n, K] on the device: the exact K nearest OTHER rows of every row of ``store_or_xf`` (an fp32 ``RefineStore``
    or a float32 device tensor [n, d]), nearest first -- ``search`` of the rows against themselves with the row itself
    removed by its junk rule (pids = the row numbers, one camera); -1 pads a row when n - 1 < K.  2 <= K <= 128."""
    _cluster_metric(metric, 'nng_knn')
    K = _int_arg(K, 2, NNG_K_MAX, 'nng_knn', 'K')
    if isinstance(store_or_xf, RefineStore):
        if store_or_xf.dtype != 'f32':
            raise ValueError("nng_knn: store_or_xf must be an 'f32' RefineStore: the exact lists are taken on the fp32 rows "
                             "(got a %r store)" % (store_or_xf.dtype,))
        xf = store_or_xf.data
    else:
        xf = _nng_store(store_or_xf, 'f32', 'nng_knn', 'store_or_xf')[0].data
    n = int(xf.shape[0])
    import numpy as np
    ids, cams = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    return search(xf, xf, K, metric, exclude=(ids, ids, cams, cams), block_bytes=block_bytes)[1]


def nng_optimize(knn, D):
    """int32 [n, D] on the device: the neighbour table of the candidate lists ``knn`` (an integer device tensor [n, K],
    row i = the candidate neighbours of i, nearest first; an entry equal to i, outside 0..n-1 or repeated is padding) --
    the graph optimisation of include/grl_hip.h: rank-based detour counts (grl_nng_detours), the first D live positions
    by (detours, position), the reverse lists by (position, source) and their merge (grl_nng_merge).  Integers only:
    tests/nng_ref.py gives the same table.  2 <= K <= 128, D even in 2..min(K, 64).  No host loop over n, nothing n x n."""
    if not (torch.is_tensor(knn) and knn.is_cuda and knn.dim() == 2 and not knn.dtype.is_floating_point
            and not knn.dtype.is_complex and knn.dtype != torch.bool):
        raise ValueError('nng_optimize: knn must be an integer device tensor [n, K] (got %s)'
                         % ((tuple(knn.shape), knn.dtype, knn.device) if torch.is_tensor(knn) else type(knn).__name__,))
    n, K = (int(v) for v in knn.shape)
    if not 2 <= K <= NNG_K_MAX:
        raise ValueError('nng_optimize: knn must have K columns with K in 2..%d (got K = %d)' % (NNG_K_MAX, K))
    if n >= 2 ** 31:
        raise ValueError('nng_optimize: knn must have fewer than 2**31 rows (got %d)' % n)
    D = _int_arg(D, 2, min(K, NNG_D_MAX), 'nng_optimize', 'D (even, 2 <= D <= min(K, %d))' % NNG_D_MAX)
    if D % 2:
        raise ValueError('nng_optimize: D must be even (got %d)' % D)
    dev = knn.device
    out = torch.full((n, D), -1, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    knn = knn.to(torch.int64)
    knn32 = torch.where((knn >= 0) & (knn < n), knn, torch.full_like(knn, -1)).to(torch.int32).contiguous()
    det = torch.empty((n, K), dtype=torch.int32, device=dev)
    _call('grl_nng_detours', ptr(knn32), ptr(det), n, K)
    # the first D live positions by (det, b): one integer sort per row
    pos = torch.arange(K, dtype=torch.int64, device=dev).view(1, K)
    pad = K * K + K
    key, order = torch.where(det >= 0, det.to(torch.int64) * K + pos, torch.full_like(pos, pad)).sort(dim=1)
    fwd = torch.where(key[:, :D] < pad, knn32.gather(1, order[:, :D]), torch.full_like(knn32[:, :D], -1)).contiguous()
    # the reverse lists in CSR form, ordered by (position in F, source): a stable sort by target of the (position, source) order
    flat = fwd.t().contiguous().view(-1)
    keep = flat >= 0
    tgt = flat[keep].to(torch.int64)
    src = torch.arange(n, dtype=torch.int32, device=dev).repeat(D)[keep]
    rev = src[torch.sort(tgt, stable=True)[1]].contiguous()
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.bincount(tgt, minlength=n).cumsum(0)
    if rev.numel() == 0:
        rev = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _call('grl_nng_merge', ptr(fwd), ptr(off), ptr(rev), ptr(out), n, D)
    return out


class NnGraphIndex(object):
    """A kNN-graph index over the rows of a feature store: ``NnGraphIndex(store, neighbors, metric)`` wraps
    the caller's ``RefineStore`` (n rows) and neighbour table ``neighbors`` (int32 device tensor [n, D], contiguous, D even
    in 2..64; an entry outside 0..n-1 is padding) without copying either.  ``n``, ``d``, ``D``, ``metric``, ``store``,
    ``neighbors``, ``nbytes`` (the table; ``nng_build`` adds the store when it made one).  ValueError names what is wrong."""

    def __init__(self, store, neighbors, metric='cosine'):
        _cluster_metric(metric, 'NnGraphIndex')
        if not isinstance(store, RefineStore):
            raise ValueError('NnGraphIndex: store must be a RefineStore (got %s)' % type(store).__name__)
        if not (torch.is_tensor(neighbors) and neighbors.dim() == 2 and neighbors.dtype == torch.int32):
            raise ValueError('NnGraphIndex: neighbors must be an int32 device tensor [n, D] (got %s)'
                             % ((tuple(neighbors.shape), neighbors.dtype) if torch.is_tensor(neighbors)
                                else type(neighbors).__name__,))
        if not neighbors.is_cuda or neighbors.device != store.data.device:
            raise ValueError('NnGraphIndex: neighbors must be on the device of the store, %s (got %s)'
                             % (store.data.device, neighbors.device))
        n, D = (int(v) for v in neighbors.shape)
        if n != store.n:
            raise ValueError('NnGraphIndex: neighbors must have one row per store row: the store has %d, neighbors %d' % (store.n, n))
        if D % 2 or not 2 <= D <= NNG_D_MAX:
            raise ValueError('NnGraphIndex: neighbors must have D columns with D even in 2..%d (got D = %d)' % (NNG_D_MAX, D))
        if not neighbors.is_contiguous():
            raise ValueError('NnGraphIndex: neighbors must be contiguous (got strides %s)' % (tuple(neighbors.stride()),))
        self.store, self.neighbors, self.metric = store, neighbors, metric
        self.n, self.d, self.D = n, store.d, D
        self.nbytes = n * D * 4


def nng_build(xf_or_store, K=64, D=32, metric='cosine', dtype='f32', knn=None):
    """The index of the rows ``xf_or_store``: a float32 device tensor [n, d] (the index then owns a ``RefineStore`` of
    ``dtype`` 'f32' | 'bf16' over it; a bf16 copy counts in ``nbytes``) or a ``RefineStore`` (used as it is; ``dtype``
    must be its own).  ``knn=None`` takes the exact lists ``nng_knn(rows, K, metric)`` of the fp32 rows; a caller brings
    approximate ones (an integer device tensor [n, K'], e.g. the lists of ``refine_search`` of the rows against their own
    index) for a large n, and K is then K'.  Equal to ``NnGraphIndex(store, nng_optimize(knn, D), metric)``."""
    _cluster_metric(metric, 'nng_build')
    if dtype not in REFINE_TYPES:
        raise ValueError("nng_build: dtype must be 'f32' or 'bf16' (got %r)" % (dtype,))
    if isinstance(xf_or_store, RefineStore):
        if xf_or_store.dtype != dtype:
            raise ValueError('nng_build: dtype must be the store\'s own, %r (got %r)' % (xf_or_store.dtype, dtype))
        store, owned = xf_or_store, False
        if knn is None and dtype != 'f32':
            raise ValueError("nng_build: knn is required with a 'bf16' RefineStore: the exact lists are taken on fp32 rows")
        rows = store.data
    else:
        store, owned = _nng_store(xf_or_store, dtype, 'nng_build', 'xf_or_store')
        rows = xf_or_store.contiguous()
    if knn is None:
        K = _int_arg(K, 2, NNG_K_MAX, 'nng_build', 'K')
        knn = nng_knn(rows, K, metric)
    elif torch.is_tensor(knn) and knn.dim() == 2 and knn.shape[0] != store.n:
        raise ValueError('nng_build: knn must have one row per store row: the store has %d, knn %d' % (store.n, knn.shape[0]))
    index = NnGraphIndex(store, nng_optimize(knn, D), metric)
    if owned:
        index.nbytes += store.nbytes
    return index


def nng_default_seeds(n, L):
    """the seeds of ``nng_search(seeds=None)``: S = min(L, n) row numbers floor(j * n / S), a python list"""
    S = min(int(L), int(n))
    return [(j * int(n)) // S for j in range(S)]


def nng_search(qf, index, k, L=64, w=1, T=64, seeds=None, exclude=None, return_stats=False):
    """Each query's ``k`` nearest rows by a beam search on the graph of ``index`` (an ``NnGraphIndex``): ``(dist [nq, k]
    float32, idx [nq, k] int64)`` on the device, and with ``return_stats`` a third value, int32 [nq, 2]: the rows visited
    (= scored) and the iterations run.  One grl_nng_search launch per block of at most 65535 queries walks the graph from
    the ``seeds`` with an itopk list of ``L`` entries (a power of two in 8..512, k <= L), ``w`` parents per iteration
    (1..8, w * D <= 256) and at most ``T`` iterations, and scores every visited row with the normative pair distance of
    ``refine_dist`` on the index's store: the lists need no second stage, and tests/nng_ref.py gives the same bits.
    ``seeds=None``: S = min(L, n) evenly spaced rows floor(j * n / S); else an integer device tensor [S] (shared) or
    [nq, S] (per query, e.g. the head of an ``ivf_search`` list), 1 <= S <= L, entries outside 0..n-1 and repeats skipped.
    ``exclude`` is the junk tuple of ``search``: junk rows are walked like any other (dropping them would cut a query off
    from its own neighbourhood) and are removed from the finished list of L, of which the first k remaining are returned;
    with fewer than k left the tail is index -1, distance +inf.  The workgroup's LDS (query row, sort buffer, visited table
    of >= 2 min(S + T * w * D, n) slots) must fit 64 KiB: ValueError names the bytes and the limit otherwise.  A
    ``verify_metric`` is refused.  Not sharded: every rank computes the full result."""
    what = 'nng_search'
    if not isinstance(index, NnGraphIndex):
        raise ValueError('%s: index must be an NnGraphIndex (got %s); a verify_metric or any other ranking is refused: the '
                         'walk scores rows by cosine or euclidean pair distances' % (what, type(index).__name__))
    store, n, D = index.store, index.n, index.D
    if not torch.is_tensor(qf) or qf.dim() != 2 or qf.shape[1] != store.d:
        raise ValueError('%s: qf must be [rows, d] = [rows, %d] (got %s)'
                         % (what, store.d, tuple(qf.shape) if torch.is_tensor(qf) else type(qf).__name__))
    require_device(qf, 'qf')
    qf = qf.contiguous()
    nq, dev = int(qf.shape[0]), qf.device
    L = _int_arg(L, NNG_L_MIN, NNG_L_MAX, what, 'L (a power of two)')
    if L & (L - 1):
        raise ValueError('%s: L must be a power of two in %d..%d (got %d)' % (what, NNG_L_MIN, NNG_L_MAX, L))
    k = _int_arg(k, 1, L, what, 'k (k <= L = %d)' % L)
    w = _int_arg(w, 1, NNG_W_MAX, what, 'w')
    if w * D > NNG_WD_MAX:
        raise ValueError('%s: w must keep w * D <= %d (got w = %d with D = %d)' % (what, NNG_WD_MAX, w, D))
    T = _int_arg(T, 1, _INT_MAX, what, 'T')
    if seeds is None:
        if n == 0:
            seeds_t, S, stride = torch.zeros(1, dtype=torch.int32, device=dev), 1, 0
        else:
            s = nng_default_seeds(n, L)
            seeds_t, S, stride = torch.tensor(s, dtype=torch.int32, device=dev), len(s), 0
    else:
        if not (torch.is_tensor(seeds) and seeds.is_cuda and seeds.dim() in (1, 2) and not seeds.dtype.is_floating_point
                and not seeds.dtype.is_complex and seeds.dtype != torch.bool):
            raise ValueError('%s: seeds must be an integer device tensor [S] or [nq, S] (got %s)'
                             % (what, (tuple(seeds.shape), seeds.dtype, seeds.device) if torch.is_tensor(seeds)
                                else type(seeds).__name__))
        if seeds.dim() == 2 and seeds.shape[0] != nq:
            raise ValueError('%s: seeds [nq, S] must have one row per query: %d (got %d)' % (what, nq, seeds.shape[0]))
        S = int(seeds.shape[-1])
        if not 1 <= S <= L:
            raise ValueError('%s: seeds must hold 1 <= S <= L = %d ids per query (got S = %d)' % (what, L, S))
        s64 = seeds.to(torch.int64)
        seeds_t = torch.where((s64 >= 0) & (s64 < n), s64, torch.full_like(s64, -1)).to(torch.int32).contiguous()
        stride = S if seeds.dim() == 2 else 0
    junk = _junk_ids(exclude, nq, n, dev)
    need = int(_lib.load().grl_nng_search_lds_bytes(n, store.d, D, L, w, T, S))
    if need > NNG_LDS_MAX:
        raise ValueError('%s: the query row, the sort buffer and the visited table of d = %d, L = %d, w = %d, T = %d, S = %d, '
                         'D = %d need %d bytes of LDS, the limit is %d (lower T, w or L)'
                         % (what, store.d, L, w, T, S, D, need, NNG_LDS_MAX))
    dist = torch.full((nq, L), float('inf'), dtype=torch.float32, device=dev)
    idx32 = torch.full((nq, L), -1, dtype=torch.int32, device=dev)
    stats = torch.zeros((nq, 2), dtype=torch.int32, device=dev)
    if nq and n:
        block = max(1, min(65535, NNG_QUERY_BLOCK))
        for q0 in range(0, nq, block):
            q1 = min(q0 + block, nq)
            _call('grl_nng_search', ptr(qf[q0:q1]), store.d, ptr(store.data), store.d, REFINE_TYPES[store.dtype],
                  ptr(index.neighbors), ptr(seeds_t[q0:] if stride else seeds_t), stride, ptr(dist[q0:q1]), ptr(idx32[q0:q1]),
                  ptr(stats[q0:q1]), q1 - q0, n, store.d, D, L, w, T, S, PQ_METRICS[index.metric])
    idx = idx32.to(torch.int64)
    if junk is not None and nq:
        q_pids, q_cams, g_pids, g_cams = junk
        safe = idx.clamp(min=0)
        drop = (idx >= 0) & (g_pids[safe] == q_pids.view(-1, 1)) & (g_cams[safe] == q_cams.view(-1, 1))
        # kept entries first, in their order (the L-list is sorted; a stable sort of the drop flag keeps it)
        order = torch.sort(drop.to(torch.int8), dim=1, stable=True)[1]
        dist = torch.where(drop, torch.full_like(dist, float('inf')), dist).gather(1, order)
        idx = torch.where(drop, torch.full_like(idx, -1), idx).gather(1, order)
    dist, idx = dist[:, :k].contiguous(), idx[:, :k].contiguous()
    return (dist, idx, stats) if return_stats else (dist, idx)


# ----------------------------------------------------------------------------
# binary hash codes (ITQ, LSH) and Hamming search on the device (bin.hip)
# ----------------------------------------------------------------------------
BIN_NBITS_MAX = 1024                                                  # GRL_BIN_NBITS_MAX of include/grl_hip.h
BIN_SLAB = 1024                                                       # GRL_BIN_SLAB: gallery columns per workgroup of grl_bin_scan
BIN_NQ_MAX = 524280                                                   # GRL_BIN_NQ_MAX: queries per grl_bin_scan call
BIN_METHODS = ('itq', 'lsh')
BIN_MODES = ('hamming', 'asymmetric')


def _bin_nbits(nbits, what):
    if isinstance(nbits, bool) or not isinstance(nbits, numbers.Integral) or nbits % 32 or not 32 <= nbits <= BIN_NBITS_MAX:
        raise ValueError('%s: nbits must be an integer multiple of 32 in 32..%d (got %r)' % (what, BIN_NBITS_MAX, nbits))
    return int(nbits)


def _bin_mode(mode, what):
    if mode not in BIN_MODES:
        raise ValueError("%s: mode must be 'hamming' or 'asymmetric' (got %r)" % (what, mode))


def _bin_mean(xp, n):
    """mu [1, dp] of the padded rows: ``pca``'s mean (cluster_centroids(xf, zeros, 1, 'mean')'s kernels)."""
    labels = torch.zeros(n, dtype=torch.int32, device=xp.device)
    counts = torch.full((1,), n, dtype=torch.int32, device=xp.device)
    return _kmeans_update(xp, labels, counts, 1, 'mean')[0]


def _bin_shift(mu, ppad):
    """shift [nbits] = -(proj mu): one GEMM row and grl_pca_affine, as ``Pca.affine`` makes its own."""
    rows = ppad.shape[0]
    cm, one, shift = (_new((rows,), ppad) for _ in range(3))
    _pca_shift(mu, ppad, rows, None, one, shift, cm)
    return shift


class BinaryCodebook(object):
    """The hyperplanes of a binary hash: ``proj`` [nbits, d] float32 on the device, ``shift`` [nbits] or
    None, nbits a multiple of 32 in 32..1024.  z = x proj^T + shift is one fp32 GEMM (exact fp32 whatever ``set_math``
    says; d is padded with zero columns to a multiple of 32 as ``Pca.transform`` pads it) and bit b of a row is z[b] > 0
    (NaN, -0 and +0 give 0).  ``metric`` is the distance a second stage refines by (``bin_refine_search``).  A caller may
    wrap a projection of its own; ``bin_train`` fills ``method`` / ``n_iter`` / ``seed`` / ``objective`` (None otherwise).
    ValueError names the argument that is wrong."""

    def __init__(self, proj, shift=None, metric='cosine'):
        what = 'BinaryCodebook'
        _cluster_metric(metric, what)
        _pca_matrix(proj, what, 'proj')
        nbits, d = int(proj.shape[0]), int(proj.shape[1])
        _bin_nbits(nbits, what)
        if d < 1:
            raise ValueError('%s: proj must be [nbits, d] with d >= 1 (got %s)' % (what, tuple(proj.shape)))
        if shift is not None and not (torch.is_tensor(shift) and shift.is_cuda and shift.dtype == torch.float32
                                      and tuple(shift.shape) == (nbits,)):
            raise ValueError('%s: shift must be None or a float32 device tensor [nbits] = [%d] (got %s)'
                             % (what, nbits, (tuple(shift.shape), shift.dtype, shift.device) if torch.is_tensor(shift)
                                else type(shift).__name__))
        self.nbits, self.d, self.metric = nbits, d, metric
        self.proj, self._ppad = proj, _pad_features(proj)
        self.shift = None if shift is None else shift.contiguous()
        self.method = self.n_iter = self.seed = self.objective = None

    def _check(self, xf, what, name):
        _pca_matrix(xf, what, name)
        if xf.shape[1] != self.d:
            raise ValueError('%s: %s must be [rows, d] = [rows, %d] (got %s)' % (what, name, self.d, tuple(xf.shape)))
        return xf

    def _rows(self, xf, what, name):
        return _pad_features(self._check(xf, what, name))

    def _project(self, xp):
        n = xp.shape[0]
        z = _new((n, self.nbits), xp)
        if n:
            gemm(xp, self._ppad, z, n, self.nbits, xp.shape[1], shift=self.shift, math=MATH_F32)
        return z

    def project(self, xf):
        """z [rows, nbits] float32: z[i, b] = (xf[i] . proj[b]) + shift[b], the fp32 GEMM's bits."""
        return self._project(self._rows(xf, 'BinaryCodebook.project', 'xf'))

    def _pack(self, z, scan=True):
        """grl_bin_pack: (codes uint8 [n, nbits / 8], scan words int32 [nbits / 32, n]) of the projections ``z``; without
        ``scan`` (query rows: the symmetric scan reads their public bytes) the words are None and are not written."""
        n = z.shape[0]
        codes = torch.empty((n, self.nbits // 8), dtype=torch.uint8, device=z.device)
        words = torch.empty((self.nbits // 32, n), dtype=torch.int32, device=z.device) if scan else None
        if n:
            _call('grl_bin_pack', ptr(z), self.nbits, ptr(codes), ptr(words), n, None, 0, n, self.nbits)
        return codes, words

    def _encode(self, xf, what='BinaryCodebook.encode'):
        return self._pack(self._project(self._rows(xf, what, 'xf')))

    def encode(self, xf):
        """uint8 [rows, nbits / 8], the public layout: bit j of byte m is ``project(xf)[:, 8 * m + j] > 0``, i.e.
        numpy.packbits(z > 0, axis=1, bitorder='little')."""
        return self._encode(xf)[0]

    def lut(self, qf):
        """The asymmetric tables [nq, nbits / 8, 256] float32 of the query projections z = project(qf): entry [q, m, c] is
        the sequential fp32 sum from +0 over j = 0..7 of -z[q, 8m + j] where bit j of c is set, +z[q, 8m + j] elsewhere
        (grl_bin_lut; tests/bin_ref.py gives the same bits)."""
        z = self._project(self._rows(qf, 'BinaryCodebook.lut', 'qf'))
        nq = z.shape[0]
        lut = _new((nq, self.nbits // 8, 256), z)
        if nq:
            _call('grl_bin_lut', ptr(z), self.nbits, ptr(lut), nq, self.nbits)
        return lut


def bin_train(xf, nbits, method='itq', n_iter=50, seed=0):
    """A ``BinaryCodebook`` of ``nbits`` hyperplanes trained on the rows of ``xf`` [n, d].  Both methods centre on the mean
    of ``xf`` (``pca``'s mean, bit for bit): shift = -(proj mean), since post-ReLU features sit far from the origin.
    'lsh': proj = Generator(PCG64(seed)).standard_normal((nbits, d)) as float32 from the host.  'itq' (iterative
    quantisation): V = pca(xf, nbits, seed=seed).transform(xf); R_0 = the float64 QR of a host Gaussian [nbits, nbits] of
    the same seed; ``n_iter`` rounds of Z = V R (the GEMM), B = sign(Z) as +-1 (grl_bin_pack), A = B^T V (the slab-reduced
    weight-gradient GEMM), R = the orthogonal Procrustes solution from the float64 SVD of A on the host (one nbits x nbits
    download and upload per round: training glue that does not grow with n); ``objective`` lists the sums of singular
    values, one per round; finally proj = R^T C by the GEMM.  pca's limits and errors apply (nbits + 10 <= min(n - 1, d,
    512)).  The same bits on every run.  Not sharded: every rank trains the full, identical codebook.  ValueError names
    the argument: ``xf`` not a 2-d float32 device tensor, method, nbits, n_iter < 1, seed < 0."""
    import numpy as np
    what = 'bin_train'
    _pca_matrix(xf, what, 'xf')
    if method not in BIN_METHODS:
        raise ValueError("%s: method must be 'itq' or 'lsh' (got %r)" % (what, method))
    c = _bin_nbits(nbits, what)
    n_iter = _kmeans_int(n_iter, 1, what, 'n_iter')
    seed = _kmeans_int(seed, 0, what, 'seed')
    n, d = int(xf.shape[0]), int(xf.shape[1])
    dev = xf.device
    if method == 'lsh':
        if n < 1 or d < 1:
            raise ValueError('%s: xf needs at least one row and one column (got %s)' % (what, tuple(xf.shape)))
        xp = _pad_features(xf)
        dp = xp.shape[1]
        ppad = torch.zeros((c, dp), dtype=torch.float32, device=dev)
        host = np.random.Generator(np.random.PCG64(seed)).standard_normal((c, d)).astype(np.float32)
        ppad[:, :d] = torch.from_numpy(host).to(dev)
        mu, objective = _bin_mean(xp, n), None
    else:
        p = pca(xf, c, seed=seed)
        cpad, mu = p._cpad, p._mu
        dp, npad = cpad.shape[1], _pad32(n)
        # v and b are padded with zero rows to a multiple of 32, as _PcaFit pads the z it hands to _pca_wgrad; only the
        # rows below n are ever rewritten, so the padding stays zero and adds +0 to B^T V
        v = torch.zeros((npad, c), dtype=torch.float32, device=dev)
        v[:n] = p.transform(xf)
        b = torch.zeros((npad, c), dtype=torch.float32, device=dev)
        z, a = _new((n, c), v), _new((c, c), v)
        g = np.random.Generator(np.random.PCG64(seed)).standard_normal((c, c))
        r = np.linalg.qr(g)[0]
        objective = []
        for _ in range(n_iter):
            rt = torch.from_numpy(np.ascontiguousarray(r.T).astype(np.float32)).to(dev)
            gemm(v, rt, z, n, c, c, math=MATH_F32)                              # Z = V R
            _call('grl_bin_pack', ptr(z), c, None, None, 0, ptr(b), c, n, c)    # B = sign(Z)
            _pca_wgrad(b, v, a, n, c, c, c)                                     # A = B^T V
            u, s, vh = np.linalg.svd(a.cpu().numpy().astype(np.float64))
            objective.append(float(s.sum()))
            r = (u @ vh).T                                                      # argmax_R tr(A R) over the orthogonal R
        rt = torch.from_numpy(np.ascontiguousarray(r.T).astype(np.float32)).to(dev)
        ct = _new((dp, c), v)
        _call('grl_transpose', ptr(cpad), ptr(ct), c, dp, dp)
        ppad = _new((c, dp), v)
        gemm(rt, ct, ppad, c, dp, c, math=MATH_F32)                             # proj = R^T C
    shift = _bin_shift(mu, ppad)
    book = BinaryCodebook(ppad[:, :d] if dp == d else ppad[:, :d].contiguous(), shift)
    book.method, book.n_iter, book.seed, book.objective = method, n_iter, seed, objective
    return book


def _bin_codes(codes, nbits, what):
    if not (torch.is_tensor(codes) and codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2
            and codes.shape[1] == nbits // 8):
        raise ValueError('%s: codes must be a uint8 device tensor [n, nbits / 8] = [n, %d] (got %s)'
                         % (what, nbits // 8, (tuple(codes.shape), codes.dtype) if torch.is_tensor(codes) else type(codes).__name__))
    return codes.contiguous()


class BinaryIndex(object):
    """A gallery as binary codes: ``codebook``, ``codes`` (uint8 [n, nbits / 8] on the device, the public layout), ``n``,
    ``nbits`` and ``nbytes`` = everything the index keeps on the device: the codes, their scan-layout copy (uint32
    [nbits / 32, n], what grl_bin_scan and grl_pq_scan read coalesced; grl_bin_words makes it from caller-supplied codes)
    and the projection with its shift."""

    def __init__(self, codebook, codes, _scan=None):
        if not isinstance(codebook, BinaryCodebook):
            raise ValueError('BinaryIndex: codebook must be a BinaryCodebook (got %s)' % type(codebook).__name__)
        self.codebook, self.nbits = codebook, codebook.nbits
        self.codes = _bin_codes(codes, codebook.nbits, 'BinaryIndex')
        self.n = int(self.codes.shape[0])
        if _scan is None:
            _scan = torch.empty((self.nbits // 32, self.n), dtype=torch.int32, device=self.codes.device)
            if self.n:
                _call('grl_bin_words', ptr(self.codes), ptr(_scan), self.n, self.n, self.nbits)
        self._scan = _scan
        self.nbytes = self.codes.numel() + 4 * _scan.numel() + 4 * codebook.proj.numel() \
            + (0 if codebook.shift is None else 4 * codebook.nbits)


def bin_index(xf, codebook):
    """``BinaryIndex(codebook, codebook.encode(xf))`` with the scan layout written by the same launch as the codes."""
    if not isinstance(codebook, BinaryCodebook):
        raise ValueError('bin_index: codebook must be a BinaryCodebook (got %s)' % type(codebook).__name__)
    codes, scan = codebook._encode(xf, 'bin_index')
    return BinaryIndex(codebook, codes, scan)


class _BinBlocks(_BlockSource):
    """Column blocks of the distance matrix of ``qf`` against the code rows of ``index``: a ``_BlockSource`` like
    ``_PqBlocks``.  'hamming': the constructor encodes
    the queries and a block is grl_bin_scan over the word rows [c0, c1) in place (the kernel takes the row stride);
    'asymmetric': the constructor makes the tables of all its queries (``codebook.lut``) and a block is grl_pq_scan with
    M = nbits / 8, ksub = 256 over a contiguous copy of the block's words.  An entry depends on its codes and its query
    alone, so a block holds the full matrix's bits whatever its width."""

    def __init__(self, qf, index, mode='hamming', block_cols=None, block_bytes=None):
        _check_index(index, BinaryIndex, '_BinBlocks')
        _bin_mode(mode, '_BinBlocks')
        book = index.codebook
        xp = book._rows(qf, '_BinBlocks', 'qf')
        self.qf, self.index, self.mode, self.ng = xp, index, mode, index.n
        self.nq = nq = xp.shape[0]
        self._cut(0, index.n, block_cols, block_bytes)
        self.qwords = self.lut = self.z = None
        if self.spans and nq:
            self.z = book._project(xp)
            if mode == 'hamming':
                self.qwords = book._pack(self.z, scan=False)[0].view(torch.int32)         # [nq, nbits / 32]: the public bytes
            else:
                self.lut = _new((nq, book.nbits // 8, 256), xp)
                _call('grl_bin_lut', ptr(self.z), book.nbits, ptr(self.lut), nq, book.nbits)

    def block(self, c0, c1):
        n, nbits, nq = c1 - c0, self.index.nbits, self.nq
        out = self._view(n)
        scan = self.index._scan
        if self.mode == 'hamming':
            for q0 in range(0, nq, BIN_NQ_MAX):
                q1 = min(q0 + BIN_NQ_MAX, nq)
                _call('grl_bin_scan', ptr(self.qwords[q0:q1]), ptr(scan[:, c0:]), self.ng, ptr(out[q0:q1]), n, q1 - q0, n, nbits)
            return out
        if n != self.ng:                                   # grl_pq_scan's row stride is its column count
            scan = scan[:, c0:c1].contiguous()
        _call('grl_pq_scan', ptr(self.lut), ptr(scan), ptr(out), nq, n, nbits // 8, 256, n, PQ_METRICS['cosine'], None)
        return out


def bin_dist(qf, index, mode='hamming', block_cols=None, block_bytes=None):
    """The materialised [nq, n] float32 distances of ``qf`` against ``index``, for small cases and tests.  'hamming': the
    number of differing bits between the query's code and the row's, an exact integer in 0..nbits.  'asymmetric':
    -sum_b z_q[b] s_g[b] with z_q the query's projection and s_g = +-1 the row's bits, as the ADC sum of include/grl_hip.h
    over ``codebook.lut(qf)`` (tests/pq_ref.adc_dist gives the same bits); smaller = nearer under both.  The same bits for
    every ``block_cols``."""
    _check_index(index, BinaryIndex, 'bin_dist')
    _bin_mode(mode, 'bin_dist')
    blocks = _BinBlocks(qf, index, mode, index.n if block_cols is None and block_bytes is None else block_cols, block_bytes)
    return _dist_from_blocks(blocks, index.n)


def _bin_query_rows(book, mode):
    """queries per block source: the grid's limit, and for 'asymmetric' the tables that fit GRL_PQ_LUT_BYTES (at least one)"""
    if mode == 'hamming':
        return BIN_NQ_MAX
    return max(1, min(PQ_NQ_MAX, PQ_LUT_BYTES // (4 * (book.nbits // 8) * 256)))


def bin_search(qf, index, k, mode='hamming', exclude=None, block_cols=None, block_bytes=None):
    """``search`` on D = bin_dist(qf, index, mode): ``(dist [nq, k] float32, idx [nq, k] int64)``, bit for bit
    ``rank_rows(D)[:, :k]`` and D at those indices, without D: blocks of code rows through grl_bin_scan ('hamming') or
    grl_pq_scan over the asymmetric tables, ranked by search's running top-k.  Hamming distances are small integers, so
    ties are the rule: they go to the smaller gallery index.  ``exclude`` is search's junk rule; padding is index -1,
    distance +inf; k <= 1024.  The asymmetric tables obey GRL_PQ_LUT_BYTES as ``pq_search``'s do: beyond it the queries
    are served in row blocks, whose results are independent and concatenated.  Not sharded."""
    _check_index(index, BinaryIndex, 'bin_search')
    _bin_mode(mode, 'bin_search')
    k, book = _search_k(k, 'bin_search'), index.codebook
    qf = book._check(qf, 'bin_search', 'qf')
    junk = _junk_ids(exclude, qf.shape[0], index.n, qf.device)
    return _search_by_query_rows(lambda q: _BinBlocks(q, index, mode, block_cols, block_bytes), qf,
                                 _bin_query_rows(book, mode), k, junk)


def bin_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids, mode='hamming', max_rank=100, block_cols=None,
                          block_bytes=None):
    """``rank_metrics(rank_rows(D), ...)`` for D = bin_dist(qf, index, mode) without D: (cmc[max_rank] float32, mAP float)
    with rank_metrics_streaming's contract.  'asymmetric': the tables of ALL queries must fit GRL_PQ_LUT_BYTES, as in
    ``pq_metrics_streaming`` (ValueError naming the bytes), and there are at most 262 140 of them (grl_pq_scan's grid).
    Not sharded."""
    _check_index(index, BinaryIndex, 'bin_metrics_streaming')
    _bin_mode(mode, 'bin_metrics_streaming')
    book = index.codebook
    qf = book._check(qf, 'bin_metrics_streaming', 'qf')
    if mode == 'asymmetric':
        need = 4 * qf.shape[0] * (book.nbits // 8) * 256
        if qf.shape[0] > PQ_NQ_MAX:
            raise ValueError('bin_metrics_streaming: at most %d queries per call in mode \'asymmetric\' (grl_pq_scan\'s grid; got '
                             '%d): evaluate the queries in parts or use mode \'hamming\'' % (PQ_NQ_MAX, qf.shape[0]))
        if need > PQ_LUT_BYTES:
            raise ValueError('bin_metrics_streaming: the query tables take %d bytes (nq * nbits / 8 * 256 * 4 = %d * %d * 256 '
                             '* 4), above GRL_PQ_LUT_BYTES = %d' % (need, qf.shape[0], book.nbits // 8, PQ_LUT_BYTES))
    blocks = _BinBlocks(qf, index, mode, block_cols, block_bytes)
    return _metrics_from_blocks(blocks, blocks.nq, index.n, q_pids, g_pids, q_camids, g_camids, max_rank, False)


def bin_refine_search(qf, index, store, k, R, mode='hamming', exclude=None, block_bytes=None):
    """Two-stage search over a ``BinaryIndex``: exactly ``refine_lists(qf, store, bin_search(qf, index, R, mode,
    exclude=exclude)[1], k, index.codebook.metric, block_bytes)``.  The junk rule is applied in the first stage and nowhere
    else.  k <= R <= 1024; store.n and store.d must be the index's.  ValueError names the argument that is wrong."""
    _check_index(index, BinaryIndex, 'bin_refine_search')
    _bin_mode(mode, 'bin_refine_search')
    book = index.codebook
    return _two_stage('bin_refine_search', qf, index, book.d, book.metric, store, k, R,
                      lambda R: bin_search(qf, index, R, mode, exclude=exclude, block_bytes=block_bytes), block_bytes)


# ----------------------------------------------------------------------------
# int8 scalar-quantised gallery searched on the integer MFMA (sq8.hip)
# ----------------------------------------------------------------------------
SQ8_D_MAX = 16384                                                     # GRL_SQ8_D_MAX of include/grl_hip.h
SQ8_TILE = 128                                                        # GRL_SQ8_TILE: the output tile of grl_sq8_scan, both ways
SQ8_NQ_MAX = 1048576                                                  # GRL_SQ8_NQ_MAX: queries per grl_sq8_scan / grl_sq8_query call


def _sq8_dpad(d):
    return -(-d // 64) * 64


def _sq8_vector(t, d, what, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and (d is None or t.shape[0] == d)):
        raise ValueError('%s: %s must be a float32 device tensor [d]%s (got %s)'
                         % (what, name, '' if d is None else ' = [%d]' % d,
                            (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    return t.contiguous()


class Sq8Codebook(object):
    """The per-column scalar quantiser of include/grl_hip.h: ``mean`` [d] and ``delta`` [d] >= 0, float32
    on the device, d <= 16384; ``inv`` [d] is kept next to them (127 / (127 delta), 0 where delta is 0; ``sq8_train`` stores
    127 / amax).  A row's code is clamp(rint((x - mean) * inv), -127, 127) per column as int8 (NaN gives 0), stored
    [rows, dpad] with dpad = d rounded up to a multiple of 64 and zero columns beyond d; its value is mean + delta * code.
    ``metric`` ('cosine' | 'euclidean') is the distance of the scan and of a second stage.  ValueError names the argument
    that is wrong."""

    def __init__(self, mean, delta, metric='cosine', _inv=None):
        what = 'Sq8Codebook'
        _cluster_metric(metric, what)
        self.mean = _sq8_vector(mean, None, what, 'mean')
        d = int(self.mean.shape[0])
        if not 1 <= d <= SQ8_D_MAX:
            raise ValueError('%s: mean must be [d] with d in 1..%d (got %s)' % (what, SQ8_D_MAX, tuple(mean.shape)))
        self.delta = _sq8_vector(delta, d, what, 'delta')
        if not bool((self.delta >= 0).all()):
            raise ValueError('%s: delta must be >= 0 in every column (and not NaN)' % what)
        self.d, self.dpad, self.metric = d, _sq8_dpad(d), metric
        if _inv is None:
            _inv = _new((d,), self.mean)
            _call('grl_sq8_steps', None, ptr(self.delta), ptr(_inv), d)
        self.inv = _inv
        self._mupad = _pad_features(self.mean.view(1, d))            # [1, dp]: the bias GEMM's row

    def _check(self, xf, what, name):
        _pca_matrix(xf, what, name)
        if xf.shape[1] != self.d:
            raise ValueError('%s: %s must be [rows, d] = [rows, %d] (got %s)' % (what, name, self.d, tuple(xf.shape)))
        return xf

    def _codes(self, codes, what):
        """caller-supplied codes as the stored layout int8 [rows, dpad]: [rows, dpad] is taken as it is (its columns >= d
        must be 0), [rows, d] is copied into zero-padded rows"""
        if not (torch.is_tensor(codes) and codes.is_cuda and codes.dtype == torch.int8 and codes.dim() == 2
                and codes.shape[1] in (self.d, self.dpad)):
            raise ValueError('%s: codes must be an int8 device tensor [rows, dpad] = [rows, %d] or [rows, d] = [rows, %d] (got %s)'
                             % (what, self.dpad, self.d,
                                (tuple(codes.shape), codes.dtype) if torch.is_tensor(codes) else type(codes).__name__))
        if codes.shape[1] == self.dpad:
            codes = codes.contiguous()
            if self.dpad > self.d and bool(codes[:, self.d:].any()):
                raise ValueError('%s: the columns d .. dpad = %d .. %d of codes must be 0' % (what, self.d, self.dpad))
            return codes
        out = torch.zeros((codes.shape[0], self.dpad), dtype=torch.int8, device=codes.device)
        out[:, :self.d] = codes
        return out

    def encode(self, xf):
        """int8 [rows, dpad], the stored layout (``[:, :d]`` is the public view): the row codes of ``xf`` [rows, d]."""
        xf = self._check(xf, 'Sq8Codebook.encode', 'xf').contiguous()
        n = xf.shape[0]
        codes = torch.empty((n, self.dpad), dtype=torch.int8, device=xf.device)
        if n:
            _call('grl_sq8_encode', ptr(xf), self.d, ptr(self.mean), ptr(self.inv), ptr(codes), self.dpad, n, self.d)
        return codes

    def _decode(self, codes, out, ldo):
        if codes.shape[0]:
            _call('grl_sq8_decode', ptr(codes), self.dpad, ptr(self.mean), ptr(self.delta), ptr(out), ldo, codes.shape[0], self.d)
        return out

    def decode(self, codes):
        """float32 [rows, d]: mean + delta * code per column (one multiply, one add), the value of a stored row."""
        codes = self._codes(codes, 'Sq8Codebook.decode')
        return self._decode(codes, _new((codes.shape[0], self.d), self.mean), self.d)

    def _query(self, qp, d):
        """(qcodes, scale, bias, qq) of query rows padded to a multiple of 32 columns (``_pad_features``)"""
        nq, dp = qp.shape
        dev = qp.device
        qcodes = torch.empty((nq, self.dpad), dtype=torch.int8, device=dev)
        scale, bias, qq = _new((nq,), qp), _new((nq,), qp), _new((nq,), qp)
        for q0 in range(0, nq, SQ8_NQ_MAX):
            q1 = min(q0 + SQ8_NQ_MAX, nq)
            _call('grl_sq8_query', ptr(qp[q0:q1]), dp, ptr(self.delta), ptr(qcodes[q0:q1]), self.dpad, ptr(scale[q0:q1]),
                  q1 - q0, d)
        if nq:
            gemm(self._mupad, qp, bias, 1, nq, dp, math=MATH_F32)             # bias[q] = q . mean: one GEMM row
            _call('grl_row_sqnorm', ptr(qp), ptr(qq), nq, dp, dp)
        return qcodes, scale, bias, qq

    def query(self, qf):
        """``(qcodes int8 [nq, dpad], scale [nq], bias [nq], qq [nq])`` of the queries ``qf`` [nq, d]: w = q * delta per
        column, s = the largest finite |w|, qcodes = clamp(rint(w * (127 / s)), -127, 127) (0 for a NaN or infinite w,
        and everywhere when s is 0), scale = s / 127; bias = q . mean by the exact-fp32 GEMM; qq = grl_row_sqnorm(q).
        The dot product of a query with a stored row is then scale * (qcodes . codes) + bias."""
        return self._query(_pad_features(self._check(qf, 'Sq8Codebook.query', 'qf')), self.d)


def sq8_train(xf, metric='cosine'):
    """The ``Sq8Codebook`` of the rows of ``xf`` [n, d]: ``mean`` = the column mean (``pca``'s and ``bin_train``'s, bit
    for bit), amax[j] = max_i |x[i][j] - mean[j]| (NaN ignored; an integer atomic maximum on the bits: no order),
    delta = amax / 127 and inv = 127 / amax (0 for a constant column).  The same bits on every run.  Not sharded: every
    rank trains the full, identical codebook."""
    what = 'sq8_train'
    _pca_matrix(xf, what, 'xf')
    _cluster_metric(metric, what)
    n, d = int(xf.shape[0]), int(xf.shape[1])
    if n < 1 or not 1 <= d <= SQ8_D_MAX:
        raise ValueError('%s: xf needs at least one row and 1..%d columns (got %s)' % (what, SQ8_D_MAX, tuple(xf.shape)))
    xp = _pad_features(xf)
    mean = _bin_mean(xp, n)[0, :d].contiguous()
    amax, delta, inv = (_new((d,), xp) for _ in range(3))
    _call('grl_sq8_absmax', ptr(xp), xp.shape[1], ptr(mean), ptr(amax), n, d)
    _call('grl_sq8_steps', ptr(amax), ptr(delta), ptr(inv), d)
    return Sq8Codebook(mean, delta, metric, _inv=inv)


class Sq8Index(object):
    """A gallery as int8 codes: ``codebook``, ``codes`` (int8 [n, dpad] on the device, zero beyond column d; ``codes[:, :d]``
    is the public view; caller-supplied codes may be [n, d] and may hold -128), ``gg`` [n] = grl_row_sqnorm of the decoded
    rows (the Euclidean epilogue's term), ``n``, ``d`` and ``nbytes`` = everything the index keeps on the device: codes, gg
    and the codebook's three vectors."""

    def __init__(self, codebook, codes):
        if not isinstance(codebook, Sq8Codebook):
            raise ValueError('Sq8Index: codebook must be a Sq8Codebook (got %s)' % type(codebook).__name__)
        self.codebook, self.d = codebook, codebook.d
        self.codes = codebook._codes(codes, 'Sq8Index')
        self.n = n = int(self.codes.shape[0])
        self.gg = _new((n,), self.codes)
        d4 = -(-self.d // 4) * 4                                      # rows grl_row_sqnorm can read; the padding stays zero
        rows = max(1, min(n, (64 << 20) // (4 * d4)))
        buf = torch.zeros((rows, d4), dtype=torch.float32, device=self.codes.device) if n else None
        for r0 in range(0, n, rows):
            r1 = min(r0 + rows, n)
            codebook._decode(self.codes[r0:r1], buf, d4)
            _call('grl_row_sqnorm', ptr(buf), ptr(self.gg[r0:]), r1 - r0, d4, d4)
        self.nbytes = self.codes.numel() + 4 * n + 12 * self.d

    def reconstruct(self, rows):
        """float32 [len(rows), d]: the stored values of the gallery rows ``rows`` (a 1-d integer device tensor)."""
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 1 and not rows.dtype.is_floating_point
                and not rows.dtype.is_complex and rows.dtype != torch.bool):
            raise ValueError('Sq8Index.reconstruct: rows must be a 1-d integer device tensor of gallery indices')
        rows = rows.to(torch.int64)
        if rows.numel() and bool(((rows < 0) | (rows >= self.n)).any()):
            raise ValueError('Sq8Index.reconstruct: rows must be in 0..n-1 = 0..%d' % (self.n - 1))
        codes = self.codes[rows].contiguous()
        return self.codebook._decode(codes, _new((codes.shape[0], self.d), self.gg), self.d)


def sq8_index(xf, codebook):
    """``Sq8Index(codebook, codebook.encode(xf))``."""
    if not isinstance(codebook, Sq8Codebook):
        raise ValueError('sq8_index: codebook must be a Sq8Codebook (got %s)' % type(codebook).__name__)
    xf = codebook._check(xf, 'sq8_index', 'xf')
    if xf.shape[0] >= 2 ** 31:
        raise ValueError('sq8_index: n must be below 2**31 (got %d)' % xf.shape[0])
    return Sq8Index(codebook, codebook.encode(xf))


class _Sq8Blocks(_BlockSource):
    """Column blocks of the distance matrix of ``qf`` against the code rows of ``index``: a ``_BlockSource`` like
    ``_PqBlocks``.  The constructor quantises the
    queries (``codebook.query``); a block is grl_sq8_scan over the code rows [c0, c1) in place (a pointer offset: the
    kernel takes the row stride).  An entry depends on its two code rows and its query's scale, bias and norm alone, and
    the integer sum has no order, so a block holds the full matrix's bits whatever its width."""

    def __init__(self, qf, index, block_cols=None, block_bytes=None):
        _check_index(index, Sq8Index, '_Sq8Blocks')
        book = index.codebook
        xp = _pad_features(book._check(qf, '_Sq8Blocks', 'qf'))
        self.qf, self.index, self.nq, self.ng = xp, index, xp.shape[0], index.n
        self._cut(0, index.n, block_cols, block_bytes)
        self.qcodes = self.scale = self.bias = self.qq = None
        if self.spans and self.nq:
            self.qcodes, self.scale, self.bias, self.qq = book._query(xp, book.d)

    def block(self, c0, c1):
        n, nq, book = c1 - c0, self.nq, self.index.codebook
        out = self._view(n)
        for q0 in range(0, nq, SQ8_NQ_MAX):
            q1 = min(q0 + SQ8_NQ_MAX, nq)
            _call('grl_sq8_scan', ptr(self.qcodes[q0:q1]), book.dpad, ptr(self.index.codes[c0:c1]), book.dpad,
                  ptr(self.scale[q0:q1]), ptr(self.bias[q0:q1]), ptr(self.qq[q0:q1]), ptr(self.index.gg[c0:c1]),
                  ptr(out[q0:q1]), n, q1 - q0, n, book.dpad, PQ_METRICS[book.metric])
        return out


def sq8_dist(qf, index, block_cols=None, block_bytes=None):
    """The materialised [nq, n] float32 distances of ``qf`` against ``index``, for small cases and tests: per pair
    dot = scale * float(qcodes . codes) + bias with the exact int32 sum; 'cosine': -dot; 'euclidean':
    sqrt(max((qq + gg) - 2 dot, 1e-12)), a NaN argument giving 1e-12 as in pairwise_distance_tensor.  tests/sq8_ref.py
    gives the same bits.  The same bits for every ``block_cols``."""
    _check_index(index, Sq8Index, 'sq8_dist')
    blocks = _Sq8Blocks(qf, index, index.n if block_cols is None and block_bytes is None else block_cols, block_bytes)
    return _dist_from_blocks(blocks, index.n)


def sq8_search(qf, index, k, exclude=None, block_cols=None, block_bytes=None):
    """``search`` on D = sq8_dist(qf, index): ``(dist [nq, k] float32, idx [nq, k] int64)``, bit for bit
    ``rank_rows(D)[:, :k]`` and D at those indices, without D: blocks of code rows through grl_sq8_scan, ranked by
    search's running top-k.  Ties go to the smaller gallery index; ``exclude`` is search's junk rule; padding is index -1,
    distance +inf; k <= 1024.  Not sharded: every rank computes the full result."""
    _check_index(index, Sq8Index, 'sq8_search')
    k = _search_k(k, 'sq8_search')
    qf = index.codebook._check(qf, 'sq8_search', 'qf')
    nq = qf.shape[0]
    junk = _junk_ids(exclude, nq, index.n, qf.device)
    blocks = _Sq8Blocks(qf, index, block_cols, block_bytes)
    return _search_blocks(blocks, nq, k, False, junk)


def sq8_metrics_streaming(qf, index, q_pids, g_pids, q_camids, g_camids, max_rank=100, block_cols=None, block_bytes=None):
    """``rank_metrics(rank_rows(D), ...)`` for D = sq8_dist(qf, index) without D: (cmc[max_rank] float32, mAP float) with
    rank_metrics_streaming's contract.  Not sharded."""
    _check_index(index, Sq8Index, 'sq8_metrics_streaming')
    qf = index.codebook._check(qf, 'sq8_metrics_streaming', 'qf')
    blocks = _Sq8Blocks(qf, index, block_cols, block_bytes)
    return _metrics_from_blocks(blocks, blocks.nq, index.n, q_pids, g_pids, q_camids, g_camids, max_rank, False)


def sq8_refine_search(qf, index, store, k, R, exclude=None, block_bytes=None):
    """Two-stage search over a ``Sq8Index``: exactly ``refine_lists(qf, store, sq8_search(qf, index, R,
    exclude=exclude)[1], k, index.codebook.metric, block_bytes)``.  The junk rule is applied in the first stage and nowhere
    else.  k <= R <= 1024; store.n and store.d must be the index's.  ValueError names the argument that is wrong."""
    _check_index(index, Sq8Index, 'sq8_refine_search')
    book = index.codebook
    return _two_stage('sq8_refine_search', qf, index, book.d, book.metric, store, k, R,
                      lambda R: sq8_search(qf, index, R, exclude=exclude, block_bytes=block_bytes), block_bytes)
