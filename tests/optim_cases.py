"""Oracles and case tables of the optimizer kernels (docs/OPTIM_SPEC.md; csrc/optim.hip:
adam_elem, radam_elem, centralize_row).

Two oracles.  The FLOAT32 oracle restates the documented arithmetic op for op in numpy float32
(the library is built with -ffp-contract=off -fno-fast-math, `/` and sqrtf are correctly
rounded, denormals are kept): the kernels must equal it bit for bit.  The FLOAT64 oracle is the
published algorithm -- torch.optim.AdamW, oracle/ref_optim.py -- on float64 tensors; the float32
oracle must stay within a few units of float32 rounding of it (tests/test_optim_oracle.py),
which ties the bitwise oracle to the algorithm and not to the kernel's text.  MUTANTS are wrong
variants of the float32 oracle; every case that claims to cover a branch must tell them apart.

No GPU and no library call in this module: the per-step scalars are computed here.
"""
import math
from collections import namedtuple

import numpy as np
import torch

F = np.float32
ONE = F(1)
STEPS = 13          # un-rectified 1-5, rectified from 6, Lookahead syncs of k=6 at 6 and 12
LR = 2e-3
EPS24 = 2.0 ** -24

# Accuracy of the float32 oracle against the float64 oracle, in units of 2^-24 x the element's
# magnitude budget of the float64 run (p, slow: |p0| + sum_t |dp_t|; m: max_t |m_t|; v, vmax:
# max_t v_t): the worst ordinary element of any tensor, step and case of the kind.  Set at
# <= 4x the value measured on the CPU (tests/test_optim_oracle.py prints it per case):
UNITS = {
    'adamw': dict(p=32.0, m=10.0, v=16.0, x=16.0),      # measured 16.14, 4.70, 7.98, 6.13 (vmax)
    'radam': dict(p=32.0, m=10.0, v=16.0, x=0.0),       # measured 13.94, 4.42, 7.98, no buffer
    'ranger': dict(p=24.0, m=14.0, v=16.0, x=24.0),     # measured 9.70, 7.17, 7.44, 8.74 (slow)
}


def f32d(x):
    """The float32 nearest to x, as a Python double: what the C ABI receives."""
    return float(F(x))


# ------------------------------------------------------------------------------ step scalars
def adam_scalars(lr, b1, b2, t):
    """What adamw_step derives from the step count: doubles at the float32 lr and betas,
    rounded to float32 once.  bc2 (not used by the kernel) serves a mutant."""
    lr, b1, b2 = f32d(lr), f32d(b1), f32d(b2)
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    return dict(lr=F(lr), step_size=F(lr / bc1), bc2_sqrt=F(math.sqrt(bc2)), bc2=F(bc2))


def radam_scalars(lr, b1, b2, t, threshold, ge_rule, degenerate, k):
    """What radam_rectify and the sync rule derive from the step count.  step_size -1: no
    update.  ge_rule: RAdam's '>=' against Ranger's '>'."""
    lr, b1, b2, thr = f32d(lr), f32d(b1), f32d(b2), f32d(threshold)
    b2t = math.pow(b2, float(t))
    nmax = 2.0 / (1.0 - b2) - 1.0
    nsma = nmax - 2.0 * t * b2t / (1.0 - b2t)
    bc1 = 1.0 - math.pow(b1, float(t))
    rectified = nsma >= thr if ge_rule else nsma > thr
    nobc2 = None
    if rectified:
        r = (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)
        step_size = F(math.sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma *
                                nmax / (nmax - 2.0)) / bc1)
        nobc2 = F(math.sqrt(r) / bc1)       # mutant: the (1 - beta2^t) moved under the root of v
    else:
        step_size = F(1.0 / bc1) if degenerate else F(-1)
    return dict(lr=F(lr), step_size=step_size, rectified=bool(rectified),
                sync=bool(k > 0 and t % k == 0), bc2=F(1.0 - b2t), step_size_nobc2=nobc2)


# ------------------------------------------------------------------------- element functions
def adam_elem(p, g, m, v, x, h, s, mut=None):
    """adam_elem of csrc/optim.hip on float32 arrays -> (p, m, v, x)."""
    lr, b1, b2, eps, wd = s['lr'], h['b1'], h['b2'], h['eps'], h['wd']
    if mut == 'coupled_decay':
        g = g + wd * p
    elif mut != 'decay_after':
        p = p * (ONE - lr * wd)
    if mut == 'lerp_swap':
        m = m * b1 + (ONE - b1) * g
    else:
        m = m + (g - m) * (ONE - b1)
    v = v * b2 + (ONE - b2) * g * g
    if h['amsgrad']:
        x = np.fmax(x, v)
        vv = x
    else:
        vv = v
    if mut == 'eps_in_root':
        denom = np.sqrt(vv + eps) / s['bc2_sqrt']
    elif mut == 'bc_before_root':
        denom = np.sqrt(vv / s['bc2']) + eps
    else:
        denom = np.sqrt(vv) / s['bc2_sqrt'] + eps
    p = p - s['step_size'] * (m / denom)
    if mut == 'decay_after':
        p = p * (ONE - lr * wd)
    return p, m, v, x


def radam_elem(p, g, m, v, x, h, s, mut=None):
    """radam_elem of csrc/optim.hip on float32 arrays -> (p, m, v, slow).  x is read and
    written on a sync step only."""
    lr, b1, b2, eps, wd = s['lr'], h['b1'], h['b2'], h['eps'], h['wd']
    step_size, rectified = s['step_size'], s['rectified']
    if mut == 'coupled_decay':
        g = g + wd * p
    v = v * b2 + (ONE - b2) * g * g
    if mut == 'lerp_swap':
        m = m + (g - m) * (ONE - b1)
    else:
        m = m * b1 + (ONE - b1) * g
    updates = rectified or step_size > 0
    decays = wd != 0 and (updates or mut == 'uncond_decay') and mut != 'coupled_decay'
    if decays and mut != 'decay_after':
        p = p - wd * lr * p
    if rectified:
        if mut == 'eps_in_root':
            p = p - step_size * lr * (m / np.sqrt(v + eps))
        elif mut == 'bc_before_root':
            p = p - s['step_size_nobc2'] * lr * (m / (np.sqrt(v / s['bc2']) + eps))
        else:
            p = p - step_size * lr * (m / (np.sqrt(v) + eps))
    elif step_size > 0:
        p = p - step_size * lr * m
    if decays and mut == 'decay_after':
        p = p - wd * lr * p
    if s['sync']:
        alpha = h['alpha']
        if mut == 'la_swapped':
            x = p + alpha * (x - p)
        else:
            x = x + alpha * (p - x)
        p = x
    return p, m, v, x


def row_mean(row):
    """The exact float64 row sum divided by the row length (as the kernel: double / double),
    rounded to float32."""
    return F(math.fsum(row.astype(np.float64).tolist()) / float(row.size))


_CENTRALISED = {}   # (id of a cached gradient, mutant) -> (the gradient, its centralisation)


def centralize(g, mut=None):
    """centralize_row over the rows of dim 0: g - float32(float64 row mean), in float32.
    Remembered for the read-only gradients of step_grads, which every case shares."""
    if g.flags.writeable:
        return _centralize(g, mut)
    key = (id(g), mut)
    if key not in _CENTRALISED:
        out = _centralize(g, mut)
        out.setflags(write=False)
        _CENTRALISED[key] = (g, out)
    return _CENTRALISED[key][1]


def _centralize(g, mut):
    rows = g.reshape(g.shape[0], -1)
    if mut == 'gc_f32_mean':
        mean = np.cumsum(rows, axis=1, dtype=F)[:, -1] / F(rows.shape[1])
    elif mut == 'gc_whole_mean':
        mean = np.full(rows.shape[0], row_mean(rows.reshape(-1)), dtype=F)
    else:
        mean = np.array([row_mean(r) for r in rows], dtype=F)
    return (rows - mean[:, None]).reshape(g.shape)


def mean_is_safe(row):
    """Whether a float64 sum of the row IN ANY ORDER gives the float32 mean of the exact sum:
    the exact mean is further than n * 2^-53 * sum|g| / n from every float32 rounding
    boundary (n - 1 additions of relative error 2^-53 each, and the division)."""
    vals = row.astype(np.float64).tolist()
    n = len(vals)
    mean = math.fsum(vals) / n
    tol = n * 2.0 ** -53 * math.fsum(abs(x) for x in vals) / n
    lo = min(mean - tol, math.nextafter(mean, -math.inf))
    hi = max(mean + tol, math.nextafter(mean, math.inf))
    return F(lo) == F(hi)


def unsafe_rows(g):
    return sum(not mean_is_safe(r) for r in g.reshape(g.shape[0], -1))


# ------------------------------------------------------------------------------- the tensors
Spec = namedtuple('Spec', 'name shape group layout offset grad')
# layout: 'flat' | 'cl' (channels_last on the device) | '2d'; offset: elements into a larger
# buffer (1, 2, 3: +4, +8, +12 bytes, the misaligned vector path); grad False: no gradient.
OFFSET_N = 1029
CONV = [(32, 5, 3, 3), (64, 130, 3, 3), (2, 32, 1, 1)]
EXTREME = 4099      # the flat tensor that carries the three slices below
ZERO = slice(64, 192)           # exact zeros
TINY = slice(1000, 1100)        # |g| ~ 1e-20: (1 - beta2) g g is a float32 denormal; crosses 1024
HUGE = slice(4080, 4099)        # |g| ~ 1e18, the vector tail included


def flat_sizes(c):
    """The vector tail, the 1024-element inner loop and the chunk edges (c elements per
    workgroup: dvsof_adamw_chunk_elems())."""
    return sorted({1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, c - 1, c, c + 1, 2 * c + 3, EXTREME})


def specs(c):
    """Group 0: the flat tensors, three misaligned views, a parameter without a gradient, a
    zero-element tensor.  Group 1: channels_last conv weights and a 2-D tensor."""
    out = [Spec(f'flat{n}', (n,), 0, 'flat', 0, True) for n in flat_sizes(c)]
    out += [Spec(f'off{4 * k}', (OFFSET_N,), 0, 'flat', k, True) for k in (1, 2, 3)]
    out += [Spec('nograd', (77,), 0, 'flat', 0, False), Spec('empty', (0,), 0, 'flat', 0, True)]
    out += [Spec('conv' + 'x'.join(map(str, s)), s, 1, 'cl', 0, True) for s in CONV]
    out += [Spec('mat16x40', (16, 40), 1, '2d', 0, True)]
    return out


def initial(sp):
    rng = np.random.default_rng(5)
    return {s.name: (rng.standard_normal(s.shape, dtype=F) * F(0.1)) for s in sp}


def ordinary(s):
    """Mask of the elements compared with the float64 oracle: the zero, denormal and 1e18
    slices are bitwise-only."""
    mask = np.ones(s.shape, dtype=bool)
    if s.shape == (EXTREME,):
        mask[ZERO] = mask[TINY] = mask[HUGE] = False
    return mask


_GRADS = {}
# one seed per step, chosen so that no centralised row of the step lies near a float32 rounding
# boundary (mean_is_safe; asserted in tests/test_optim_oracle.py)
GRAD_SEEDS = [1201, 1002, 1003, 1004, 1005, 1006, 1207, 1008, 1009, 1010, 1111, 1112, 1113]


def step_grads(sp, t, huge=True):
    """Seeded normal gradients that grow with the step (1-based); None without a gradient.
    huge False: the 1e18 slice stays ordinary (under a guard it would own the norm).
    Computed once and shared: the arrays are read-only."""
    key = (tuple(sp), t, huge)
    if key not in _GRADS:
        _GRADS[key] = _step_grads(sp, t, huge)
    return _GRADS[key]


def _step_grads(sp, t, huge):
    out = {}
    for s in sp:
        # a stream per tensor: the values of one do not depend on the rest of the table
        rng = np.random.default_rng([GRAD_SEEDS[t - 1], s.offset, *s.shape])
        g = rng.standard_normal(s.shape, dtype=F) * F(1 + 0.1 * t)
        if s.shape == (EXTREME,):
            g[ZERO] = 0
            g[TINY] *= F(1e-20)
            if huge:
                g[HUGE] *= F(1e18)
        g.setflags(write=False)
        out[s.name] = g if s.grad else None
    return out


def ref_scale(grads, max_norm):
    """float32(max_norm / (float64 norm + 1e-6)): the guard's clip scale to within an ulp."""
    sq = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values() if g is not None)
    return F(min(1.0, max_norm / (math.sqrt(sq) + 1e-6)))


# --------------------------------------------------------------------------------- the cases
DEFAULTS = {
    'adamw': dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False),
    'radam': dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True),
    'ranger': dict(lr=LR, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5,
                   weight_decay=0, use_gc=True, gc_conv_only=False),
}
Case = namedtuple('Case', 'name kind hyper group_lr')


def _case(name, kind, group_lr=None, **hyper):
    return Case(name, kind, dict(DEFAULTS[kind], **hyper), group_lr)


CASES = [
    _case('adamw-ams-wd0', 'adamw', amsgrad=True, weight_decay=0),
    _case('adamw-ams-wd', 'adamw', amsgrad=True),
    _case('adamw-noams-wd0', 'adamw', weight_decay=0),
    _case('adamw-noams-wd', 'adamw'),
    _case('radam-wd0-sgd', 'radam'),
    _case('radam-wd-sgd', 'radam', weight_decay=1e-2),
    _case('radam-wd0-nosgd', 'radam', degenerated_to_sgd=False),
    _case('radam-wd-nosgd', 'radam', weight_decay=1e-2, degenerated_to_sgd=False),
    _case('ranger-default', 'ranger'),
    _case('ranger-wd', 'ranger', weight_decay=1e-2),
    _case('ranger-nogc', 'ranger', use_gc=False),
    _case('ranger-gcconv', 'ranger', gc_conv_only=True),
    _case('ranger-k1', 'ranger', k=1),
    _case('ranger-k4-a08', 'ranger', k=4, alpha=0.8),
    # two parameter groups with their own learning rate, one of them 0
    _case('adamw-groups', 'adamw', group_lr=(5e-4, 0.0), amsgrad=True),
    _case('radam-groups', 'radam', group_lr=(5e-4, 0.0), weight_decay=1e-2),
    _case('ranger-groups', 'ranger', group_lr=(5e-4, 0.0), weight_decay=1e-2),
    # a second beta pair
    _case('adamw-betas', 'adamw', amsgrad=True, betas=(0.9, 0.99)),
    _case('radam-betas', 'radam', betas=(0.9, 0.99)),
    _case('ranger-betas', 'ranger', betas=(0.9, 0.99)),
]
BY_NAME = {c.name: c for c in CASES}
BETAS = sorted({c.hyper['betas'] for c in CASES})
# the table-driven path (begin_capture / advance / step, no graph) and the guarded path
DYN_CASES = ['adamw-ams-wd', 'radam-wd-nosgd', 'ranger-wd']
GUARD_CASES = ['adamw-ams-wd', 'radam-wd-sgd', 'ranger-wd']
MAX_NORM = 100.0    # the smallest step norm of the table is ~ 1.1 * sqrt(9e4) = 330: binds always


def group_hyper(case, gi):
    h = dict(case.hyper)
    if case.group_lr is not None:
        h['lr'] = case.group_lr[gi]
    return h


def param_groups(case, tensors, sp):
    """The optimizer's `params` argument over `tensors` (name -> tensor): one group per
    Spec.group, with its learning rate where the case sets one."""
    groups = []
    for gi in (0, 1):
        g = {'params': [tensors[s.name] for s in sp if s.group == gi]}
        if case.group_lr is not None:
            g['lr'] = case.group_lr[gi]
        groups.append(g)
    return groups


def centralised(case, s):
    """Whether the case centralises the gradient of this tensor."""
    h = case.hyper
    return case.kind == 'ranger' and h['use_gc'] and len(s.shape) > (3 if h['gc_conv_only'] else 1)


# ------------------------------------------------------------------------------- the mutants
MUTANTS = ['eps', 'eps_in_root', 'bc_before_root', 'lerp_swap', 'coupled_decay', 'decay_after',
           'uncond_decay', 'sync_early', 'sync_late', 'la_swapped', 'gc_f32_mean',
           'gc_whole_mean', 'clip_first']


def covers(mut, case, guarded=False):
    """Whether `case` claims to tell this mutant from the oracle."""
    h, ranger = case.hyper, case.kind == 'ranger'
    if mut in ('eps', 'eps_in_root', 'bc_before_root', 'lerp_swap'):
        return True
    if mut in ('coupled_decay', 'decay_after'):
        return h['weight_decay'] != 0
    if mut == 'uncond_decay':
        return case.kind == 'radam' and h['weight_decay'] != 0 and not h['degenerated_to_sgd']
    if mut in ('sync_early', 'sync_late'):
        return ranger and h['k'] > 1        # k = 1 synchronises on every step either way
    if mut == 'la_swapped':
        return ranger
    if mut in ('gc_f32_mean', 'gc_whole_mean'):
        return ranger and h['use_gc']
    if mut == 'clip_first':
        return ranger and h['use_gc'] and guarded
    raise KeyError(mut)


# --------------------------------------------------------------------------- float32 oracle
class Oracle32:
    """The float32 oracle of one case: p, m, v, x (vmax / slow) per tensor, logical layout;
    `g` holds the gradient as the step leaves it in p.grad (centralised under Ranger)."""

    def __init__(self, case, sp, p0, mutant=None):
        self.case, self.sp, self.mutant, self.t = case, sp, mutant, 0
        self.p = {s.name: p0[s.name].copy() for s in sp}
        self.m = {s.name: np.zeros(s.shape, F) for s in sp}
        self.v = {s.name: np.zeros(s.shape, F) for s in sp}
        ranger = case.kind == 'ranger'
        self.x = {s.name: p0[s.name].copy() if ranger else np.zeros(s.shape, F) for s in sp}
        self.g = {}
        self.scalars = []       # per step: the scalars of each group

    def _hyper(self, gi):
        h = group_hyper(self.case, gi)
        eps = h['eps']
        if self.mutant == 'eps':
            eps = 1e-8 if eps == 1e-5 else 1e-5
        return dict(h, lr=F(h['lr']), b1=F(h['betas'][0]), b2=F(h['betas'][1]), eps=F(eps),
                    wd=F(h['weight_decay']), alpha=F(h.get('alpha', 0)))

    def _scalars(self, h):
        t, kind = self.t, self.case.kind
        if kind == 'adamw':
            return adam_scalars(h['lr'], h['b1'], h['b2'], t)
        if kind == 'radam':
            return radam_scalars(h['lr'], h['b1'], h['b2'], t, 5.0, True,
                                 h['degenerated_to_sgd'], 0)
        s = radam_scalars(h['lr'], h['b1'], h['b2'], t, h['N_sma_threshhold'], False, True, h['k'])
        if self.mutant in ('sync_early', 'sync_late'):
            s['sync'] = (t + (1 if self.mutant == 'sync_early' else -1)) % h['k'] == 0
        return s

    def step(self, grads, scale=None):
        """One step with these gradients (name -> float32 array or None); scale: the clip
        scale of a guarded step, the float32 read from the guard record."""
        self.t += 1
        mut, kind = self.mutant, self.case.kind
        hs = [self._hyper(gi) for gi in (0, 1)]
        ss = [self._scalars(h) for h in hs]
        self.scalars.append(ss)
        elem = adam_elem if kind == 'adamw' else radam_elem
        for s in self.sp:
            g = grads[s.name]
            if g is None:
                continue
            if scale is not None and mut == 'clip_first':
                g = g * scale
            if centralised(self.case, s):
                g = centralize(g, mut)
            self.g[s.name] = g
            if scale is not None and mut != 'clip_first':
                g = g * scale
            n = s.name
            with np.errstate(all='ignore'):
                self.p[n], self.m[n], self.v[n], self.x[n] = elem(
                    self.p[n], g, self.m[n], self.v[n], self.x[n], hs[s.group], ss[s.group], mut)

    def arrays(self, name):
        return dict(p=self.p[name], m=self.m[name], v=self.v[name], x=self.x[name])


# --------------------------------------------------------------------------- float64 oracle
class Oracle64:
    """The published algorithms on float64 tensors, at the float32 values of the
    hyper-parameters (the C ABI takes them as float32: at the Python double 0.999 itself
    1 - beta2 moves by 1e-5 relative, a property of the ABI and not of the arithmetic)."""

    def __init__(self, case, sp, p0):
        from oracle.ref_optim import RefRAdam, RefRanger
        self.case, self.sp = case, [s for s in sp if s.grad]
        self.t = {s.name: torch.from_numpy(p0[s.name].astype(np.float64)).requires_grad_(True)
                  for s in self.sp}
        self.opts = []
        for gi in (0, 1):
            h = group_hyper(case, gi)
            kw = {k: (tuple(f32d(b) for b in v) if k == 'betas' else
                      f32d(v) if k in ('lr', 'eps', 'weight_decay', 'alpha') else v)
                  for k, v in h.items()}
            ps = [self.t[s.name] for s in self.sp if s.group == gi]
            cls = {'adamw': torch.optim.AdamW, 'radam': RefRAdam, 'ranger': RefRanger}[case.kind]
            self.opts.append((cls(ps, **kw), ps))

    def step(self, grads):
        for s in self.sp:
            self.t[s.name].grad = torch.from_numpy(grads[s.name].astype(np.float64))
        for opt, _ in self.opts:
            opt.step()

    def arrays(self, name):
        """p, m, v, x as float64 numpy; x None where the variant has no such buffer."""
        t = self.t[name]
        for opt, ps in self.opts:
            for i, q in enumerate(ps):
                if q is not t:
                    continue
                if self.case.kind == 'adamw':
                    st = opt.state[q]
                    m, v, x = st['exp_avg'], st['exp_avg_sq'], st.get('max_exp_avg_sq')
                else:
                    m, v, x = opt.m[i], opt.v[i], getattr(opt, 'slow', None)
                    x = None if x is None else x[i]
                return dict(p=t.detach().numpy().copy(), m=m.numpy().copy(), v=v.numpy().copy(),
                            x=None if x is None else x.numpy().copy())
        raise KeyError(name)


# -------------------------------------------------------------- centralisation on its own
GC_ROWS = 3
GC_SHAPES = [(GC_ROWS, 1, 1, 1), (GC_ROWS, 2, 1, 1), (GC_ROWS, 5, 3, 3), (GC_ROWS, 7, 3, 3),
             (GC_ROWS, 16, 2, 2), (GC_ROWS, 85, 1, 3), (GC_ROWS, 64, 2, 2), (GC_ROWS, 257, 1, 1),
             (GC_ROWS, 130, 3, 3), (GC_ROWS, 256, 3, 3)]
GC_ROW_LENGTHS = [1, 2, 45, 63, 64, 255, 256, 257, 1170, 2304]
GC_VECTOR = 300     # a 1-D tensor next to them: no row of it is in any table


def gc_grads(kind):
    """'dyadic': multiples of 2^-12 with |g| < 2^11 around a common offset of 317.25 -- every
    float64 partial sum of a row is exact in any order, the result is bitwise by construction.
    'normal': seeded normal values, under mean_is_safe (asserted in test_optim_oracle.py)."""
    rng = np.random.default_rng({'dyadic': 77, 'normal': 75}[kind])
    out = []
    for s in GC_SHAPES + [(GC_VECTOR,)]:
        if kind == 'dyadic':
            g = (rng.integers(-2 ** 20, 2 ** 20, s).astype(np.float64) * 2.0 ** -12 + 317.25)
            assert np.abs(g).max() < 2 ** 11 and np.array_equal(g.astype(F).astype(np.float64), g)
            out.append(g.astype(F))
        else:
            out.append(rng.standard_normal(s, dtype=F) * F(1.7))
    return out
