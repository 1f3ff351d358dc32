"""The eval variants of gemm_f32_kernel (gemm_f32.hip EV_AFFINE / EV_SQDIFF: descriptor fields an inference launch never
sets are compile-time constants) against the generic kernel: every case runs one descriptor twice in one process, with
GRL_GEMM_EVAL_VARIANT=0 (generic) and with it unset, and the outputs must be the same bits.  Which kernel took a launch
is read from the line the library writes to stderr under GRL_DEBUG_SYNC."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = 'GRL_GEMM_EVAL_VARIANT'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    from grl_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture
def named(monkeypatch):
    """The library names every gemm_f32 launch on stderr (read per call)."""
    monkeypatch.setenv('GRL_DEBUG_SYNC', '1')
    monkeypatch.delenv(SWITCH, raising=False)


def _variants(capfd):
    return re.findall(r'gemm_f32_kernel<(\d+),(\d+),conv=(\d).*?> variant=([\w-]+)', capfd.readouterr().err)


def _both(call, capfd, tile=None):
    """call() under the generic kernel and under the default routing -> (y_generic, y_default, variant names of the second run)"""
    from grl_amd import _lib
    lib = _lib.load()
    lib.grl_gemm_force_tile(*(tile or (0, 0)))
    try:
        os.environ[SWITCH] = '0'
        capfd.readouterr()
        y0 = call()
        torch.cuda.synchronize()
        off = _variants(capfd)
        assert off and all(v[3] == 'generic' for v in off), off
        del os.environ[SWITCH]
        y1 = call()
        torch.cuda.synchronize()
        on = _variants(capfd)
        if tile:
            assert all((int(v[0]), int(v[1])) == tuple(tile) for v in off + on), (tile, off, on)
    finally:
        os.environ.pop(SWITCH, None)
        lib.grl_gemm_force_tile(0, 0)
    return y0, y1, [v[3] for v in on]


def _rand(rng, shape, dev, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dev)


def test_eval_variant_is_taken(dev, named, capfd):
    """The comparison below is not generic against generic: a plain K >= 256 affine launch on a 128-row tile runs the eval
    variant, and the switch sends it back to the generic kernel."""
    from grl_amd import engine
    rng = np.random.default_rng(0)
    M, N, K = 256, 128, 256
    a, w = _rand(rng, (M, K), dev), _rand(rng, (N, K), dev, 0.1)

    def call():
        y = torch.full((M, N), 7.0, device=dev)
        return engine.gemm(a, w, y, M, N, K, relu=True)
    for tile in ((128, 128), (128, 64)):
        y0, y1, on = _both(call, capfd, tile)
        assert on == ['eval'], (tile, on)
        assert torch.equal(y0, y1), tile


@pytest.mark.parametrize('tile', [(128, 128), (128, 64), (64, 64)])
def test_tiles_and_ragged_edges(dev, named, capfd, tile):
    """One and two stages (K = 32, 64: below the LDS-DMA threshold, generic either way), 8 and 17 stages on the eval variant,
    ragged last row and column tiles.  The 64 x 64 tile always routes to the generic kernel."""
    from grl_amd import engine
    rng = np.random.default_rng(tile[0] + tile[1])
    a_all, w_all = _rand(rng, (384, 544), dev), _rand(rng, (256, 544), dev, 0.1)
    res_all = _rand(rng, (384, 256), dev)
    for M, N, K in itertools.product((128, 129, 384), (64, 128, 132, 256), (32, 64, 256, 544)):
        a, w = a_all[:M, :K].contiguous(), w_all[:N, :K].contiguous()
        res = res_all[:M, :N].contiguous()

        def call():
            y = torch.full((M, N), 7.0, device=dev)
            return engine.gemm(a, w, y, M, N, K, res=res, relu=True)
        y0, y1, on = _both(call, capfd, tile)
        assert on == ['eval' if tile[0] == 128 and K >= 256 else 'generic'], (tile, M, N, K, on)
        assert torch.equal(y0, y1), (tile, M, N, K)


@pytest.mark.parametrize('tile', [(128, 128), (128, 64)])
def test_feature_combinations(dev, named, capfd, tile):
    """res (ldres != N) x relu x scale x gbias (groups of 32, 48, 128 rows: 48 does not divide the tile), and an unaligned y,
    which takes the scalar epilogue; M and N end inside a tile."""
    from grl_amd import engine
    rng = np.random.default_rng(11 + tile[1])
    M, N, K, ldres = 384 - 8, 136, 256, 144
    a, w = _rand(rng, (M, K), dev), _rand(rng, (N, K), dev, 0.1)
    scale, shift = torch.rand(N, device=dev) + 0.5, _rand(rng, (N,), dev)
    res = _rand(rng, (M, ldres), dev)
    gb = _rand(rng, ((M + 31) // 32, N), dev)
    ybuf = torch.empty(M * N + 4, device=dev)
    for has_res, relu, has_scale, rpg, unaligned in itertools.product((False, True), (False, True), (False, True),
                                                                     (0, 32, 48, 128), (False, True)):
        if unaligned and rpg not in (0, 48):
            continue
        kw = dict(relu=relu, shift=shift)
        if has_res:
            kw.update(res=res, ldres=ldres)
        if has_scale:
            kw.update(scale=scale)
        if rpg:
            kw.update(gbias=gb, rows_per_group=rpg)

        def call():
            ybuf.fill_(7.0)
            y = ybuf[1:1 + M * N].view(M, N) if unaligned else ybuf[:M * N].view(M, N)
            return engine.gemm(a, w, y, M, N, K, **kw).clone()
        y0, y1, on = _both(call, capfd, tile)
        assert on == ['eval'], (tile, kw.keys(), on)
        assert torch.equal(y0, y1), (tile, has_res, relu, has_scale, rpg, unaligned)
        assert not bool((y1 == 7.0).all())


@pytest.mark.parametrize('K', [64, 256])
def test_sqdiff(dev, named, capfd, K):
    """The TRL step's squared-difference epilogue (K = 64 stays below the LDS-DMA threshold: generic; K = 256: its own variant)."""
    from grl_amd import engine
    from grl_amd._lib import EPI_SQDIFF
    rng = np.random.default_rng(K)
    M, N, rr = 256, 128, 32
    a, w = _rand(rng, (M, K), dev), _rand(rng, (N, K), dev, 0.1)
    shift = _rand(rng, (N,), dev)
    f2 = torch.relu(_rand(rng, (M // rr * 2 * rr, N), dev))

    def call():
        y = torch.full((M // 32, N), 7.0, device=dev)
        return engine.gemm(a, w, y, M, N, K, shift=shift, epilogue=EPI_SQDIFF, res=f2, res_rows=rr, res_gstride=2 * rr)
    y0, y1, on = _both(call, capfd)
    assert on == ['eval-sqdiff' if K >= 256 else 'generic'], on
    assert torch.equal(y0, y1)


@pytest.mark.parametrize('tile', [(128, 128), (128, 64)])
def test_conv(dev, named, capfd, tile):
    """Implicit-GEMM windows with every tap-mask case at the image border: 3x3 stride 1 pad 1 on 4x4 images, 3x3 stride 2 pad 1
    on 8x4, 1x1 stride 2."""
    from grl_amd import engine
    rng = np.random.default_rng(5 + tile[1])
    for n, H, W, cin, cout, k, stride, pad in [(2, 4, 4, 32, 64, 3, 1, 1), (3, 8, 4, 64, 64, 3, 2, 1), (2, 8, 4, 32, 64, 1, 2, 0)]:
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        x, w = _rand(rng, (n, H, W, cin), dev), _rand(rng, (cout, k * k * cin), dev, 0.1)
        shift = _rand(rng, (cout,), dev)
        M, K = n * Ho * Wo, k * k * cin

        def call():
            y = torch.full((M, cout), 7.0, device=dev)
            return engine.gemm(x, w, y, M, cout, K, shift=shift, relu=True, conv=(H, W, cin, Ho, Wo, k, k, stride, pad))
        y0, y1, on = _both(call, capfd, tile)
        assert on == ['eval'], (tile, k, stride, on)
        assert torch.equal(y0, y1), (tile, n, H, W, cin, k, stride)


def test_routing_keeps_other_descriptors_generic(dev, named, capfd):
    """stats, rowscale, kblock and NEGDOT are outside the eval variants' feature set."""
    from grl_amd import engine
    from grl_amd._lib import EPI_NEGDOT
    rng = np.random.default_rng(3)
    M, N, K = 256, 128, 1024
    a, w = _rand(rng, (M, K), dev), _rand(rng, (N, K), dev, 0.1)
    rowscale = torch.rand(M, device=dev) + 0.5
    engine_splitk = engine.SPLITK
    engine.SPLITK = False          # (kblock at M <= 256 would otherwise leave through the split-K kernels, which name nothing)
    try:
        for kw in (dict(stats=True), dict(rowscale=rowscale), dict(kblock=True), dict(epilogue=EPI_NEGDOT)):
            def call():
                y = torch.full((M, N), 7.0, device=dev)
                out = engine.gemm(a, w, y, M, N, K, **kw)
                return torch.cat([t.reshape(-1) for t in out]) if isinstance(out, tuple) else out
            y0, y1, on = _both(call, capfd, (128, 128))
            assert on == ['generic'], (list(kw), on)
            assert torch.equal(y0, y1), list(kw)
    finally:
        engine.SPLITK = engine_splitk


_CHILD = '''
import hashlib, os, sys, torch
sys.path.insert(0, %r)
from grl_amd import engine, _lib
_lib.load().grl_gemm_force_tile(128, 128)
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(1)
for K in (64, 256):
    M, N = 2048, 128
    a = torch.randn(M, K, generator=g).to(dev); w = (torch.randn(N, K, generator=g) * 0.1).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    y = torch.full((M, N), 7.0, device=dev)
    engine.gemm(a, w, y, M, N, K, res=res, relu=True)
    print('K%%d %%s' %% (K, hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()))
'''


def test_persistent_loop_several_tiles_per_workgroup(dev):
    """GRL_GEMM_GRID=8 (read once: child processes): 16 row tiles on 8 persistent workgroups, the next tile's first stage
    requested behind the epilogue.  The same child with the variant off must print the same digests."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for off in (True, False):
        env = dict(os.environ, GRL_GEMM_GRID='8', GRL_DEBUG_SYNC='1')
        env.pop(SWITCH, None)
        if off:
            env[SWITCH] = '0'
        r = subprocess.run([sys.executable, '-c', _CHILD % root], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        names = re.findall(r'variant=([\w-]+)', r.stderr)
        assert names == (['generic', 'generic'] if off else ['generic', 'eval']), names
        outs.append(r.stdout.split())
    assert len(outs[0]) == 4 and outs[0] == outs[1], outs
