#!/usr/bin/env python
"""Launch trace of the eval forward (engine.extract_features, synthetic weights and clips): one line per launch, and per
case a sha256 of that text and a sha256 of the returned features' bytes.  Two trees that print the same table issue the
same launches with the same arguments on the same streams and compute the same bits -- the check for a host-side
refactor of the launch schedule.

A line holds: the ordinal of the current stream (first-seen order within the case), the entry point and
  * engine._call: every scalar argument; a pointer argument (``_lib._SIGNATURES``) as null / non-null only;
  * engine.gemm: M N K, the leading dimensions, epilogue, relu, conv, the math the descriptor gets, kblock,
    rows_per_group, res_rows, res_gstride, out_f32, the dtypes of a / w / y and which optional operands are present;
  * engine.gemm_group: the member problems; the fused bottleneck tails: M P C4 Pn Kd; engine.conv3x3_c64_bf16: its shape.

Cases: math f32 / bf16 / bf16x3 / bf16s / mxfp8 x clips 8x4, 32x4, 6x8, 3x8 x float32 / raw uint8 input x TRL_STREAMS
on / off; for f32 and bf16s at 8x4 every fusion / stream switch off, one at a time; grl_forward with taps for f32 (all
taps in the output digest) and bf16s (outputs, corr_map, f_uncorr, f_corr).  Every case runs once untraced first, so
that weight caches are filled outside the trace.

To compare against another checkout, run this same file with PYTHONPATH at that checkout (and GRL_HIP_LIB at the built
library, if that checkout has none):

  python tools/eval_launch_trace.py [--out table.txt] [--dump DIR] [--only SUBSTRING]
"""
import argparse
import contextlib
import ctypes as C
import hashlib
import inspect
import io
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (after PYTHONPATH: see above)

SWITCHES = ('FUSE_BNECK', 'FUSE_DOWN', 'FUSE_C64', 'FUSE_STEM_POOL', 'FUSE_STEM_POOL_F32', 'FUSE_TRL_SQDIFF', 'TRL_ATT_STREAMS')
GEMM_OPERANDS = ('scale', 'shift', 'res', 'gbias', 'rowscale', 'rnorm', 'cnorm', 'stats', 'bn')


def _scalar(v):
    v = getattr(v, 'value', v)
    return repr(float(v)) if isinstance(v, float) else repr(int(v))


class Trace(object):
    """Wraps the engine's launch wrappers (module attributes, as the forward looks them up at call time)."""
    NAMES = ('_call', 'gemm', 'gemm_group', 'bneck_tail_bf16', 'bneck_tail_f32', 'conv3x3_c64_bf16')

    def __init__(self, engine, _lib):
        self.engine, self._lib = engine, _lib
        self.orig = {n: getattr(engine, n) for n in self.NAMES}
        self.gemm_sig = inspect.signature(self.orig['gemm'])
        self.lines, self.streams = [], {}

    def add(self, text):
        s = torch.cuda.current_stream().cuda_stream
        self.lines.append('s%d %s' % (self.streams.setdefault(s, len(self.streams)), text))

    def _call(self, name, *args):
        argtypes = self._lib._SIGNATURES[name][0]
        assert len(argtypes) == len(args) + 1, name               # (+ the stream)
        self.add('%s %s' % (name, ' '.join(('p' if a else '0') if ty is C.c_void_p else _scalar(a)
                                            for ty, a in zip(argtypes, args))))
        return self.orig['_call'](name, *args)

    def _math(self, m):
        e = self.engine
        return (e.MATH_F32 if e._math[0] in (e.MATH_BF16S, e.MATH_MXFP8) else e._math[0]) if m is None else m

    def gemm(self, *args, **kw):
        p = self.gemm_sig.bind(*args, **kw)
        p.apply_defaults()
        a = p.arguments
        M, N, K = a['M'], a['N'], a['K']
        self.add('gemm %d %d %d lda %d ldw %d ldy %d ldres %d epi %d relu %d conv %s math %d kblock %d rpg %d res_rows %d '
                 'res_gstride %d out_f32 %d a %s w %s y %s with %s' % (
                     M, N, K, a['lda'] or K, a['ldw'] or K, a['ldy'] or N, a['ldres'] or N, a['epilogue'], bool(a['relu']),
                     tuple(a['conv']) if a['conv'] is not None else None, self._math(a['math']), bool(a['kblock']),
                     a['rows_per_group'], a['res_rows'], a['res_gstride'], bool(a['out_f32']), a['a'].dtype, a['w'].dtype,
                     a['y'].dtype, ','.join(k for k in GEMM_OPERANDS if a[k] is not None)))
        return self.orig['gemm'](*args, **kw)

    def gemm_group(self, calls):
        self.add('gemm_group %s' % ' | '.join('%d %d %d math %d' % (c['M'], c['N'], c['K'], self._math(c.get('math')))
                                              for c in calls))
        return self.orig['gemm_group'](calls)

    def _tail(self, name):
        def tail(t2, c3, res, c1n, M, **kw):
            down = kw.get('down')
            self.add('%s M %d P %d C4 %d Pn %d Kd %d res %d t2 %s' % (
                name, M, c3.K, c3.N, c1n.N if c1n is not None else 0, down.K if down is not None else 0,
                res is not None, t2.dtype))
            return self.orig[name](t2, c3, res, c1n, M, **kw)
        return tail

    def conv3x3_c64_bf16(self, x, c, n_img, H, W, relu=True):
        self.add('conv3x3_c64_bf16 n %d H %d W %d relu %d' % (n_img, H, W, bool(relu)))
        return self.orig['conv3x3_c64_bf16'](x, c, n_img, H, W, relu)

    @contextlib.contextmanager
    def recording(self):
        e = self.engine
        self.lines, self.streams = [], {}
        e._call, e.gemm, e.gemm_group, e.conv3x3_c64_bf16 = self._call, self.gemm, self.gemm_group, self.conv3x3_c64_bf16
        e.bneck_tail_bf16, e.bneck_tail_f32 = self._tail('bneck_tail_bf16'), self._tail('bneck_tail_f32')
        try:
            yield
        finally:
            for n, f in self.orig.items():
                setattr(e, n, f)


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def _tap_tensors(out, taps, keys=None):
    ts = list(out)
    for k in sorted(taps) if keys is None else keys:
        ts.extend(taps[k] if isinstance(taps[k], list) else [taps[k]])
    return ts


def cases():
    """(name, math, (b, t), raw uint8?, {switch: value}, taps: None | 'all' | tuple of keys)"""
    for math in ('f32', 'bf16', 'bf16x3', 'bf16s', 'mxfp8'):
        for bt in ((8, 4), (32, 4), (6, 8), (3, 8)):
            for raw in (False, True):
                for streams in (True, False):
                    yield ('%s %dx%d %s streams=%d' % (math, bt[0], bt[1], 'u8' if raw else 'f32in', streams), math, bt, raw,
                           {'TRL_STREAMS': streams}, None)
    for math in ('f32', 'bf16s'):
        for sw in SWITCHES:
            yield '%s 8x4 %s=0' % (math, sw), math, (8, 4), False, {sw: False}, None
    yield 'f32 8x4 taps', 'f32', (8, 4), False, {}, 'all'
    yield 'bf16s 8x4 taps(outputs, corr_map, f_uncorr, f_corr)', 'bf16s', (8, 4), False, {}, ('corr_map', 'f_uncorr', 'f_corr')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='write the digest table here too')
    ap.add_argument('--dump', default=None, help='directory for the full trace text of every case')
    ap.add_argument('--only', default=None, help='run the cases whose name contains this')
    args = ap.parse_args()
    from grl_amd import engine, _lib
    from grl_amd.reid import models
    from grl_amd.synthetic import synth_state_dict, synth_clips
    dev = torch.device('cuda:0')
    _lib.load()
    with contextlib.redirect_stdout(io.StringIO()):
        cnn = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=625, pretrained=False)
    siam = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    cnn.load_state_dict(synth_state_dict(cnn, seed=0))
    siam.load_state_dict(synth_state_dict(siam, seed=0, prefix='siamese.'))
    cnn.to(dev).eval()
    siam.to(dev).eval()
    tr = Trace(engine, _lib)
    table = []
    for name, math, (b, t), raw, switches, taps in cases():
        if args.only and args.only not in name:
            continue
        clips = synth_clips(b, t, seed=b * 100 + t, raw=raw).to(dev)
        old = {k: getattr(engine, k) for k in switches}
        for k, v in switches.items():
            setattr(engine, k, v)
        try:
            with (engine.experimental_math(math) if math == 'mxfp8' else engine.math_mode(math)):
                def run():
                    if taps is None:
                        return [engine.extract_features(cnn, siam, clips)]
                    tp = {}
                    return _tap_tensors(engine.grl_forward(cnn, clips, taps=tp), tp, None if taps == 'all' else taps)
                run()
                with tr.recording():
                    out = run()
                torch.cuda.synchronize()
        finally:
            for k, v in old.items():
                setattr(engine, k, v)
        text = '\n'.join(tr.lines) + '\n'
        row = '%-52s launches %4d streams %d trace %s out %s' % (
            name, len(tr.lines), len(tr.streams), hashlib.sha256(text.encode()).hexdigest()[:16], _digest(out)[:16])
        print(row, flush=True)
        table.append(row)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, ''.join(ch if ch.isalnum() else '_' for ch in name) + '.txt'), 'w') as f:
                f.write(text)
    total = 'all cases: %s' % hashlib.sha256('\n'.join(table).encode()).hexdigest()
    print(total)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(table + [total]) + '\n')


if __name__ == '__main__':
    main()
