"""The instance-contrast kernels (grl_amd/csrc/ins_contrast.hip) restated: the float64 model of the cosines, the
selection, the two softmaxes, the loss, the coefficients and the gradient; an fp32 restatement of the discrete part (the
selection from a given fp32 cos matrix, first-index ties) and of the ordered sums; the cases and the per-element bounds --
shared by test_ins_contrast_cpu.py (no GPU) and test_gpu_ins_contrast.py.

  u_i = f_i / max(|f_i|, 1e-12),  v_j = m_j / max(|m_j|, 1e-12),  c_ij = <u_i, v_j>,  t_ij = <v_i, v_j>
  K_i: one column per distinct id -- of the anchor's id (i included) the smallest c_ij (the hard positive p_i), of every other id
       the largest, the lowest index among equals
  P = softmax_K(c / tau),  Q = softmax_K(t / tau_t),  L_i = - w_hard log P_p - w_soft sum_k Q_k log P_k
  g_ik = w_hard (P_k - [k = p_i]) + w_soft (P_k - Q_k)                                  (= (w_hard + w_soft) P_k - w_hard [k = p] - w_soft Q_k)
  gu_i = (1 / tau) sum_k g_ik v_k,   df_i = dloss_i (gu_i - u_i <u_i, gu_i>) / max(|f_i|, 1e-12);  df_i = 0 where |f_i| < 1e-12

tau, tau_t, w_hard, w_soft are the fp32 values the kernel receives.  Bounds are derived per element the way loss_bounds and
soft_triplet_ref derive theirs, none is fitted: depth of the fp32 chain x u x sum|terms| (every * and + rounds once), the error
of a stage that feeds the next carried through the derivative, EXPF_ULP / DIV_ULP / LOGF_ULP / SQRT_ULP as they stand, SAFETY
once at the end, TINY wherever a result may fall under the smallest normal.

  c     d = <f_i, m_j> by one wave (k_wave_dot: product, dot4, the lane's trips of 256 floats, 6 shuffle levels) on sum|f m|; the
        inverse norms e_inv_norm of a wave dot; c = fl(fl(d inv_f) inv_m): 2 u |c|.  t likewise from m_i.
  x     fl(c / tau): DIV_ULP ulp |x| (+ e_c / tau end to end);  dd = fl(x - max): e_x + e_x(max) + u |dd|
  e     expf(dd): e (e_dd + EXPF_ULP ulp);   S: sum e_e + (|K| - 1) u S (the zeros outside K add exactly)
  nl    fl(logf(S) - dd): e_S / S + LOGF_ULP ulp |log S| + e_dd + u |nl|;   P = fl(e / S): e_e / S + P e_S / S + DIV_ULP ulp P
  Q     the same chain from t and tau_t; t is no output, so its bound enters every stage-wise check of Q
  L     fl(fl(w_h nl_p) + fl(w_s A)),  A = sum_k fl(Q_k nl_k) ascending: |K| - 1 additions
  g     fl(fl(w_h fl(P - [k = p])) + fl(w_s fl(P - Q)))
  df    w_k = fl(g inv_m_k);  acc = sum_k fl(m_k w_k): (terms) u sum|m w| + sum |m| e_w;  gu = fl(acc fl(1 / tau));  u = fl(f inv_f);
        dot = block dot of u gu (k_block_dot);  r = fl(fl(fl(gu - fl(u dot)) inv_f) dloss)"""
import numpy as np

from loss_bounds import (U, ULP, SAFETY, TINY, EXPF_ULP, DIV_ULP, LOGF_ULP, rng_for, f32, check, dump_ratios,   # noqa: F401
                         RATIOS, e_inv_norm, k_block_dot, block_dot_f32)
from head_bounds import k_wave_dot, wave_dot_f32
from head_ref import f64

F = np.float32
EPS = 1e-12
MAX_N = 2048                                    # the cap of the forward's LDS layout

# (n, D, ids): the smallest shapes that reach each path
CASES = ((2, 4, 'one'), (2, 4, 'two'), (5, 8, 'singleton'), (8, 260, 'x4'), (33, 2048, 'pairs'), (130, 4, 'pairs'),
         (9, 12, 'distinct'))
CLASSES = ('a', 't', 'z')                       # generic / tied rows / a zero student row
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (1.0, 0.4))
TAUS = ((0.1, 0.1), (0.05, 0.1))                # (tau, tau_t)
WIDE = ('plain', 'wide')                        # 'wide': negative ids, ids > 2^31, ids that differ in the high word only


def ins_ids(n, pattern, wide='plain'):
    i = np.arange(n, dtype=np.int64)
    if pattern == 'one':
        y = np.full(n, 11, np.int64)
    elif pattern == 'two':
        y = i % 2 * 4 + 5
    elif pattern == 'singleton':
        y = np.where(i == 0, 999, (i - 1) // 2 + 40)
    elif pattern == 'x4':
        y = i % 4 + 40
    elif pattern == 'pairs':
        y = i // 2 + 40
    else:
        y = i * 7 + 3
    if wide == 'wide':                          # an injective map: the partition is the same
        k = y - y.min()
        y = np.where(k % 3 == 0, -7 - k, np.where(k % 3 == 1, 5 + (k << 32), (1 << 31) + 5 + k)).astype(np.int64)
    return y


def in_ins(n, D, cls, pattern, wide='plain', seed=0):
    """f standard normal, m = f + 0.5 N(0, 1) (the teacher sees the same samples), dloss in [0.5, 1.5].
    (t) student row 1 = row 0 bit for bit with different teacher rows, and teacher row 3 = row 2, the last = row 0: equal
    columns, inside an id and across ids;  (z) student row 0 is zero: its whole cos row is 0 and every column ties."""
    r = rng_for('ins', n, D, cls, pattern, seed)
    f = f32(r.standard_normal((n, D)))
    m = f32(f + 0.5 * r.standard_normal((n, D)))
    if cls == 't':
        f[1] = f[0]
        for dst, src in ((3, 2), (n - 1, 0)):
            if 0 <= src < dst < n and dst != 1:         # (teacher rows 0 and 1 stay different)
                m[dst] = m[src]
    if cls == 'z':
        f[0] = 0.0
    return dict(f=f, m=m, ids=ins_ids(n, pattern, wide), dloss=f32(r.uniform(0.5, 1.5, n)))


def scal(v):
    """a scalar as the kernel receives it"""
    return float(F(v))


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
def norms(x):
    x = f64(x)
    ss = (x * x).sum(1)
    return ss, 1.0 / np.maximum(np.sqrt(ss), EPS)


def cosines(f, m):
    """c, t and what their bounds need"""
    f, m = f64(f), f64(m)
    ssf, invf = norms(f)
    ssm, invm = norms(m)
    d, dt = f @ m.T, m @ m.T
    return dict(ssf=ssf, invf=invf, ssm=ssm, invm=invm, d=d, dt=dt, abs_d=np.abs(f) @ np.abs(m).T, abs_dt=np.abs(m) @ np.abs(m).T,
                c=d * invf[:, None] * invm[None, :], t=dt * invm[:, None] * invm[None, :])


def select(c, ids):
    """sel [n][n]: 0 / 1 a selected negative / 2 the hard positive, from the matrix c AS GIVEN (float64, or the kernel's fp32
    cos: comparisons are exact in either): per anchor and id the smallest c of the anchor's id, the largest of every other,
    the first index among equals."""
    n = c.shape[0]
    y = np.asarray(ids, np.int64).reshape(-1)[:n]
    sel = np.zeros((n, n), np.int32)
    r = np.arange(n)
    for v in sorted(set(y.tolist())):
        g = np.flatnonzero(y == v)                                          # ascending columns
        own = y == v                                                        # per anchor
        k = np.where(own, np.argmin(c[:, g], 1), np.argmax(c[:, g], 1))    # numpy: the first index at the extreme
        sel[r, g[k]] = np.where(own, 2, 1)
    return sel


def gaps(c, ids):
    """per anchor the smallest margin by which a winner beats the runner-up of its id (inf where every id has one member)"""
    n = c.shape[0]
    y = np.asarray(ids, np.int64).reshape(-1)[:n]
    out = np.full(n, np.inf)
    for v in sorted(set(y.tolist())):
        g = np.flatnonzero(y == v)
        if g.size > 1:
            rows = np.sort(c[:, g], 1)
            out = np.minimum(out, np.where(y == v, rows[:, 1] - rows[:, 0], rows[:, -1] - rows[:, -2]))
    return out


def _softmax_parts(x, on):
    """x [n][n], on the selected mask: dd = x - rowmax over K, e, S, P (0 outside K)"""
    mx = np.where(on, x, -np.inf).max(1)
    dd = np.where(on, x - mx[:, None], 0.0)
    e = np.where(on, np.exp(dd), 0.0)
    S = e.sum(1)
    return dict(mx=mx, dd=dd, e=e, S=S, P=e / S[:, None], logS=np.log(S), imax=np.where(on, x, -np.inf).argmax(1))


def ins_forward(c, t, sel, tau, tau_t, wh, ws):
    """loss and g in float64 AT A GIVEN c, t and selection (the kernel's fp32 cos and sel stage-wise, the float64 ones end to end)"""
    c, sel = f64(c), np.asarray(sel)
    n = c.shape[0]
    on, pos = sel > 0, sel == 2
    tau, tau_t, wh, ws = scal(tau), scal(tau_t), scal(wh), scal(ws)
    x = c / tau
    s = _softmax_parts(x, on)
    nl = np.where(on, s['logS'][:, None] - s['dd'], 0.0)
    hard = (nl * pos).sum(1)
    out = dict(on=on, pos=pos, K=on.sum(1), x=x, s=s, nl=nl, hard=hard, tau=tau, tau_t=tau_t, wh=wh, ws=ws)
    g = wh * np.where(on, s['P'] - pos, 0.0)
    loss = wh * hard
    if ws != 0:
        y = f64(t) / tau_t
        q = _softmax_parts(y, on)
        term = q['P'] * nl
        A = term.sum(1)
        g = g + ws * np.where(on, s['P'] - q['P'], 0.0)
        loss = loss + ws * A
        out.update(y=y, q=q, term=term, A=A)
    out.update(g=g, loss=loss)
    return out


def ins_backward(f, m, coef, dloss, tau):
    """df in float64 at a given coef (the kernel's fp32 one stage-wise), and what its bound needs"""
    f, m, g = f64(f), f64(m), f64(coef)
    n, D = f.shape
    tau = scal(tau)
    ssf, invf = norms(f)
    ssm, invm = norms(m)
    w = g * invm[None, :]
    acc = w @ m
    gu = acc / tau
    u = f * invf[:, None]
    dot = (u * gu).sum(1)
    diff = gu - u * dot[:, None]
    dl = f64(dloss).reshape(-1)[:n]
    clamped = np.sqrt(ssf) < EPS
    df = np.where(clamped[:, None], 0.0, diff * invf[:, None] * dl[:, None])
    return dict(ssf=ssf, invf=invf, ssm=ssm, invm=invm, w=w, acc=acc, abs_acc=np.abs(w) @ np.abs(m), gu=gu, u=u, dot=dot,
                abs_dot=(np.abs(u) * np.abs(gu)).sum(1), diff=diff, dl=dl, clamped=clamped, df=df, g=g, m=m, f=f, tau=tau,
                terms=(g != 0).sum(1))


def ins_full(f, m, ids, tau, tau_t, wh, ws, dloss):
    """end to end in float64"""
    cs = cosines(f, m)
    sel = select(cs['c'], ids)
    fw = ins_forward(cs['c'], cs['t'], sel, tau, tau_t, wh, ws)
    bw = ins_backward(f, m, fw['g'], dloss, tau)
    return cs, sel, fw, bw


# ----------------------------------------------------------------------------------------------------------------------
# bounds (no SAFETY inside the e_*; the b_* carry it)
def e_inv(ss, D):
    """1 / max(sqrtf(ss), 1e-12f) from a wave dot; under the clamp it is the constant's rounding"""
    ss = np.asarray(ss, np.float64)
    safe = np.maximum(ss, EPS * EPS)
    return np.where(np.sqrt(ss) < EPS, (U + DIV_ULP * ULP) / EPS, e_inv_norm(safe, k_wave_dot(D) * U * safe))


def e_cos(cs, D, teacher=False):
    """c (or t, teacher=True) given the rows"""
    d, ad = (cs['dt'], cs['abs_dt']) if teacher else (cs['d'], cs['abs_d'])
    inv_l = cs['invm'] if teacher else cs['invf']
    e_l = e_inv(cs['ssm'] if teacher else cs['ssf'], D)
    e_r = e_inv(cs['ssm'], D)
    val = cs['t'] if teacher else cs['c']
    return (k_wave_dot(D) * U * ad * inv_l[:, None] * cs['invm'][None, :]
            + np.abs(d) * (e_l[:, None] * cs['invm'][None, :] + inv_l[:, None] * e_r[None, :]) + 2 * U * np.abs(val))


def gap_ok(cs, ids, D):
    """the condition under which the fp32 selection must equal the float64 one: every anchor's winners beat the runners-up of
    their ids by more than twice the bound on cos (the row's largest)"""
    return gaps(cs['c'], ids) > 2 * SAFETY * e_cos(cs, D).max(1)


def _e_softmax(x, s, on, tau, e_in):
    """errors of dd, e, S, log S, P along one softmax chain; e_in: what the similarity itself carries (0 when it was read)"""
    r = np.arange(x.shape[0])
    e_x = e_in / tau + DIV_ULP * ULP * np.abs(x)
    e_dd = np.where(on, e_x + e_x[r, s['imax']][:, None] + U * np.abs(s['dd']), 0.0)
    e_e = np.where(on, s['e'] * (e_dd + EXPF_ULP * ULP) + TINY, 0.0)
    K = on.sum(1)
    e_S = e_e.sum(1) + (K - 1) * U * s['S']
    e_logS = e_S / s['S'] + LOGF_ULP * ULP * np.abs(s['logS'])
    e_P = np.where(on, e_e / s['S'][:, None] + s['P'] * (e_S / s['S'])[:, None] + DIV_ULP * ULP * s['P'] + TINY, 0.0)
    return dict(e_dd=e_dd, e_S=e_S, e_logS=e_logS, e_P=e_P)


def e_forward(fw, e_t, e_c=0.0):
    """{loss, g} first-order errors.  e_c = 0: given the cos it read (stage-wise); e_t: the teacher similarities' own bound
    (t is no output: it always enters)."""
    on, pos, s, wh, ws = fw['on'], fw['pos'], fw['s'], fw['wh'], fw['ws']
    a = _e_softmax(fw['x'], s, on, fw['tau'], np.broadcast_to(np.asarray(e_c, np.float64), fw['x'].shape))
    e_nl = np.where(on, a['e_logS'][:, None] + a['e_dd'] + U * np.abs(fw['nl']), 0.0)
    pm = np.where(on, np.abs(s['P'] - pos), 0.0)
    e_g = wh * (a['e_P'] + U * pm) + U * wh * pm
    e_hard = (e_nl * pos).sum(1)
    e_loss = wh * e_hard + U * np.abs(wh * fw['hard'])
    if ws != 0:
        q = fw['q']
        b = _e_softmax(fw['y'], q, on, fw['tau_t'], e_t)
        e_term = np.where(on, b['e_P'] * np.abs(fw['nl']) + q['P'] * e_nl + U * np.abs(fw['term']) + TINY, 0.0)
        e_A = e_term.sum(1) + (fw['K'] - 1) * U * np.abs(fw['term']).sum(1)
        e_loss = e_loss + ws * e_A + U * np.abs(ws * fw['A']) + U * np.abs(fw['loss'])
        pq = np.where(on, np.abs(s['P'] - q['P']), 0.0)
        e_g = e_g + ws * (a['e_P'] + b['e_P'] + U * pq) + U * ws * pq + U * np.abs(fw['g'])
    return dict(loss=e_loss + TINY, g=np.where(on, e_g + TINY, 0.0))


def e_backward(bw, D, e_g=0.0):
    """df's first-order error.  e_g = 0: given the coef it read (stage-wise)."""
    m, f = bw['m'], bw['f']
    e_im, e_if = e_inv(bw['ssm'], D), e_inv(bw['ssf'], D)
    e_w = np.abs(bw['g']) * e_im[None, :] + U * np.abs(bw['w']) + np.asarray(e_g) * bw['invm'][None, :] + TINY * (bw['g'] != 0)
    e_acc = e_w @ np.abs(m) + bw['terms'][:, None] * U * bw['abs_acc']
    rt = 1.0 / bw['tau']
    e_gu = e_acc * rt + np.abs(bw['gu']) * (DIV_ULP * ULP + U)
    e_u = np.abs(f) * e_if[:, None] + U * np.abs(bw['u'])
    e_dot = (np.abs(bw['gu']) * e_u + np.abs(bw['u']) * e_gu).sum(1) + k_block_dot(D) * U * bw['abs_dot']
    ud = bw['u'] * bw['dot'][:, None]
    e_ud = np.abs(bw['dot'])[:, None] * e_u + np.abs(bw['u']) * e_dot[:, None] + U * np.abs(ud)
    e_diff = e_gu + e_ud + U * (np.abs(bw['gu']) + np.abs(ud))
    di = bw['diff'] * bw['invf'][:, None]
    e_r = (e_diff * bw['invf'][:, None] + np.abs(bw['diff']) * e_if[:, None] + U * np.abs(di)) * np.abs(bw['dl'])[:, None] \
        + U * np.abs(bw['df'])
    return np.where(bw['clamped'][:, None], 0.0, e_r) + TINY


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatement (numpy, CPU) of both kernels in their order; numpy's exp / log stand in for the device's expf / logf
def _inv_f32(ss):
    return F(1) / np.maximum(np.sqrt(ss), F(1e-12))


def cos_f32(f, m, teacher=False):
    f, m = F(f), F(m)
    left = m if teacher else f
    inv_l, inv_m = _inv_f32(wave_dot_f32(left, left)), _inv_f32(wave_dot_f32(m, m))
    d = wave_dot_f32(left[:, None, :], m[None, :, :])
    out = (d * inv_l[:, None]) * inv_m[None, :]
    assert out.dtype == F
    return out


def ins_f32(f, m, ids, tau, tau_t, wh, ws, dloss):
    f, m = F(f), F(m)
    n, D = f.shape
    tau, tau_t, wh, ws = F(tau), F(tau_t), F(wh), F(ws)
    c = cos_f32(f, m)
    sel = select(c, ids)
    on, pos = sel > 0, sel == 2

    def chain(v, temp):
        x = v / temp
        mx = np.where(on, x, F(-np.inf)).max(1)
        dd = x - mx[:, None]
        e = np.where(on, np.exp(np.where(on, dd, F(0))).astype(F), F(0))
        S = np.zeros(n, F)
        for k in range(n):
            S = S + e[:, k]
        return dd, e, S
    dd, e, S = chain(c, tau)
    logS = np.log(S).astype(F)
    P = e / S[:, None]
    nl = logS[:, None] - dd
    g = np.where(on, wh * (P - pos.astype(F)), F(0))
    loss = wh * np.where(pos, nl, F(0)).sum(1, dtype=F)                 # one non-zero term: exact
    if ws != 0:
        _, et, T = chain(cos_f32(f, m, teacher=True), tau_t)
        Q = et / T[:, None]
        term = np.where(on, Q * nl, F(0))
        A = np.zeros(n, F)
        for k in range(n):
            A = A + term[:, k]
        g = np.where(on, g + ws * (P - Q), F(0))
        loss = loss + ws * A
    assert g.dtype == F and loss.dtype == F
    # backward
    nf = np.sqrt(wave_dot_f32(f, f))
    invf = F(1) / np.maximum(nf, F(1e-12))
    w = g * _inv_f32(wave_dot_f32(m, m))[None, :]
    acc = np.zeros((n, D), F)
    for k in range(n):
        acc = acc + m[k][None, :] * w[:, k, None]                       # (a zero w adds exactly)
    gu = acc * (F(1) / tau)
    u = f * invf[:, None]
    dot = block_dot_f32(u, gu)
    df = ((gu - u * dot[:, None]) * invf[:, None]) * F(dloss).reshape(-1)[:n, None]
    df = np.where((nf < F(1e-12))[:, None], F(0), df)
    assert df.dtype == F
    return dict(cos=c, sel=sel, loss=loss, coef=g, df=df)


# ----------------------------------------------------------------------------------------------------------------------
# the checks both test files run: `got` holds fp32 cos [n][n], sel [n][n], loss [n], coef [n][n], df [n][D]
def check_stagewise(got, d, tau, tau_t, wh, ws, n, D, what):
    """cos against the float64 cosines; sel EQUAL to the fp32 restatement applied to got's own cos; loss and coef against the
    model at got's sel and cos; sum_k coef = 0; df against the model at got's coef"""
    cs = cosines(d['f'], d['m'])
    check('ins cos', got['cos'], cs['c'], SAFETY * e_cos(cs, D), what)
    assert np.array_equal(got['sel'], select(got['cos'], d['ids'])), ('sel', what)
    fw = ins_forward(got['cos'], cs['t'], got['sel'], tau, tau_t, wh, ws)
    e = e_forward(fw, e_cos(cs, D, teacher=True))
    check('ins loss', got['loss'], fw['loss'], SAFETY * e['loss'], what)
    check('ins coef', got['coef'], fw['g'], SAFETY * e['g'], what)
    assert (got['coef'][got['sel'] == 0] == 0).all(), ('coef outside the selection', what)
    check('ins sum coef', f64(got['coef']).sum(1), np.zeros(n), SAFETY * e['g'].sum(1), what)
    bw = ins_backward(d['f'], d['m'], got['coef'], d['dloss'], tau)
    check('ins dfeat', got['df'], bw['df'], SAFETY * e_backward(bw, D), what)
    return fw


def check_end_to_end(got, d, tau, tau_t, wh, ws, n, D, what):
    """nothing taken from the fp32 side: under the gap condition sel equals the float64 selection; loss, coef and df inside
    the bounds that carry the cosines' errors through"""
    cs, sel, fw, bw = ins_full(d['f'], d['m'], d['ids'], tau, tau_t, wh, ws, d['dloss'])
    assert gap_ok(cs, d['ids'], D).all(), ('gap', what)
    assert np.array_equal(got['sel'], sel), ('end to end sel', what)
    e = e_forward(fw, e_cos(cs, D, teacher=True), e_cos(cs, D))
    check('end to end ins loss', got['loss'], fw['loss'], SAFETY * e['loss'], what)
    check('end to end ins coef', got['coef'], fw['g'], SAFETY * e['g'], what)
    check('end to end ins dfeat', got['df'], bw['df'], SAFETY * e_backward(bw, D, e['g']), what)
