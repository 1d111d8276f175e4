"""ULTR_OPT_ADAM (csrc/ultr_update.hip: adam_step, update_body) restated in numpy, on top of loss_ref's float64 restatement of the
update launch (step_scalars: normaliser, l2 term, clip).  The law is torch.optim.Adam with its defaults:

    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)

applied to the gradient Adagrad / SGD get; state = m[P] | v[P], and for DLA m_aux[L + 1] | v_aux[L + 1] behind them, stepped with
propensity_learning_rate under the propensity clip.

step64() is the yardstick (float64), step32() the same law evaluated in float32 the way a float32 implementation has to (every
operand and every operation rounded): the distance between the two on the test inputs is the rounding FLOOR the GPU bar is derived
from.  flat_cases() / tiled_cases() are those inputs, shared by tests/test_adam_cpu.py (which measures the floor) and
tests/test_gpu_adam.py (which holds the GPU to four times it).

Measured floor and bar: see FLOOR_MEASURED / BAR below (profiles/adam.md has the table)."""
import functools

import numpy as np

from tests.loss_ref import TAIL_FIXED, hyper_of, l2_sums_of, step_scalars

B1, B2, EPS = 0.9, 0.999, 1e-8  # include/ultr_hip.h: ULTR_ADAM_BETA1 / _BETA2 / _EPS

# max |p32 - p64| / max(|p64|, lr) over every step of every case of flat_cases() and tiled_cases(), parameters, moments excluded
# (test_adam_cpu.py::test_float32_floor_is_the_recorded_one measures it again and fails if it moved).  The GPU gets four times it:
# another operation order (lr / bc1 folded on the host, one reciprocal square root for the second correction), fma contraction and
# the rounding of sqrt and the division.  The project's parity bar is 1e-5; the Adam bar must stay below it.
FLOOR_MEASURED = 5.4e-7   # 5.35e-7 (tiled-512x256x128, t = 1000); the flat cases: 4.5e-7 (flat-pdgd-P1000-clip0-l20, t = 2^31)
BAR = 4.0 * FLOOR_MEASURED  # 2.16e-6
# the moments are held too, relative to max(|m'|, |m|, the terms this step adds) (moment_excess); measured the same way: 3.95e-7
MOMENT_FLOOR_MEASURED = 4.0e-7
MOMENT_RTOL = 4.0 * MOMENT_FLOOR_MEASURED


def adam_hyper(algo, **kw):
    """loss_ref.hyper_of with Adam's eps in the adagrad_eps slot, as the engines set it."""
    h = hyper_of(algo, **kw)
    h["optimizer"] = "adam"
    h["adagrad_eps"] = float(np.float32(EPS))
    return h


def _scalars(p, g_raw, tail, ss, hyper):
    """step_scalars for the algorithms of the update launch, PDGD included: its D is 1 whatever the tail holds, and it keeps the
    clip with l2_loss > 0 (csrc/ultr_update.hip update_body)."""
    tail = np.asarray(tail, np.float64).copy()
    if hyper["algo"] == "pdgd":
        tail[1] = 1.0
    sc = step_scalars(tail, float(ss), hyper, l2_sums_of(p, g_raw) if hyper["l2_loss"] > 0 else None)
    if hyper["algo"] == "pdgd" and hyper["l2_loss"] > 0 and hyper["max_gradient_norm"] > 0:
        sc["coef"] = min(1.0, hyper["max_gradient_norm"] / (sc["norm"] + 1e-6))
    return sc


def dla_aux_grad(tail, aux, hyper, dtype=np.float64):
    """The clipped gradient of DLA's propensity parameters [W_0 .. W_{L-1}, bias] (block 0 of the update launch, as
    loss_ref.tail_update restates it): dW_l = ELU'(W_l + bias) s_l / D_exam, dbias = sum_l dW_l, x min(1, max_norm / (norm + 1e-6)).
    Returns (gradient, gross): gross is the sum of the magnitudes of each entry's terms - |dW_l|, and sum_l |dW_l| for the bias, whose
    terms may cancel (for a softmax exam loss the s_l of a list sum to zero)."""
    f = dtype
    tail, aux = np.asarray(tail, f), np.asarray(aux, f)
    L = (len(tail) - TAIL_FIXED) // 2
    z = aux[:L] + aux[L]
    g = (tail[TAIL_FIXED:TAIL_FIXED + L] / tail[3]) * np.where(z > 0, f(1.0), np.exp(np.minimum(z, f(0.0))))
    gsum = g.sum(dtype=f)
    pnorm = np.sqrt((g * g).sum(dtype=f) + gsum * gsum)
    mg = f(hyper["max_gradient_norm"])
    pc = min(f(1.0), mg / (pnorm + f(1e-6))) if mg > 0 else f(1.0)
    gross = np.concatenate([np.abs(g), np.asarray([np.abs(g).sum(dtype=f)], f)]) * pc
    return np.concatenate([g * pc, np.asarray([gsum * pc], f)]).astype(f), gross.astype(f)


def adam64(p, g, m, v, t, lr, eps):
    """One Adam step in float64, as torch.optim.Adam forms it (_single_tensor_adam): (p', m', v')."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m2 = B1 * m + (1.0 - B1) * g
    v2 = B2 * v + (1.0 - B2) * g * g
    bc1, bc2 = 1.0 - B1 ** float(t), 1.0 - B2 ** float(t)
    return p - (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)), m2, v2


def adam32(p, g, m, v, t, lr, eps):
    """The same step with every operand and every operation in float32 (the corrections are functions of t alone and are formed in
    double, then rounded): what separates it from adam64 is float32 rounding and nothing else."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    m2 = f(B1) * m + f(1.0 - B1) * g
    v2 = f(B2) * v + f(1.0 - B2) * (g * g)
    bc1, bc2 = 1.0 - B1 ** float(t), 1.0 - B2 ** float(t)
    step, sq2 = f(float(lr) / bc1), f(np.sqrt(bc2))
    return p - step * (m2 / (np.sqrt(v2) / sq2 + f(eps))), m2, v2


def _grad(p, g_raw, tail, ss, hyper, dtype):
    """(g, |terms|): the gradient the optimizer gets, g_raw gs (+ lam p), x coef, and the sum of the magnitudes of its terms."""
    f = dtype
    sc = _scalars(p, g_raw, tail, ss, hyper)
    g = np.asarray(g_raw, f) * f(sc["gs"])
    terms = np.abs(g)
    if sc["lam"] != 0.0:
        g = g + f(sc["lam"]) * np.asarray(p, f)
        terms = terms + np.abs(f(sc["lam"]) * np.asarray(p, f))
    return g * f(sc["coef"]), terms * f(sc["coef"])


def _step(adam, dtype, p, g_raw, state, t, hyper, tail, aux=None, ss=None):
    """(p', state', aux', terms) of one update launch with ULTR_OPT_ADAM on the RAW gradient (x D) and the step tail.  ss: the sum of squares
    of the raw gradient (None: formed here, in `dtype`).  terms [as state]: per moment, the magnitude of what this step adds to it,
    (1 - b1) |g| and (1 - b2) g^2 with |g| the sum of the magnitudes of the gradient's terms (moment_excess)."""
    f = dtype
    P = len(p)
    state = np.asarray(state, f)
    if ss is None:
        ss = (np.asarray(g_raw, f) ** 2).sum(dtype=f)
    g, gabs = _grad(p, g_raw, tail, ss, hyper, f)
    pn, mn, vn = adam(p, g, state[:P], state[P:2 * P], t, hyper["learning_rate"], hyper["adagrad_eps"])
    new_state, new_aux = [mn, vn], None if aux is None else np.asarray(aux, f).copy()
    terms = [(1.0 - B1) * gabs, (1.0 - B2) * gabs * gabs]
    if hyper["algo"] == "dla":
        L = len(aux) - 1
        ga, gross = dla_aux_grad(tail, aux, hyper, f)
        ma, va = state[2 * P:2 * P + L + 1], state[2 * P + L + 1:]
        new_aux, ma2, va2 = adam(aux, ga, ma, va, t, hyper["propensity_learning_rate"], hyper["adagrad_eps"])
        new_state += [ma2, va2]
        terms += [(1.0 - B1) * gross, (1.0 - B2) * gross * gross]
    return pn, np.concatenate(new_state), new_aux, np.concatenate(terms).astype(np.float64)


def step64(p, g_raw, state, t, hyper, tail, aux=None, ss=None):
    return _step(adam64, np.float64, p, g_raw, state, t, hyper, tail, aux, ss)


def step32(p, g_raw, state, t, hyper, tail, aux=None, ss=None):
    return _step(adam32, np.float32, p, g_raw, state, t, hyper, tail, aux, ss)


def state_floats(algo, P, L):
    return 2 * P + (2 * (L + 1) if algo == "dla" else 0)


def excess(got, ref, lr, cond=None):
    """max |got - ref| / max(|ref|, lr): to be held against BAR (inf for a non-finite value).  cond: per entry, the condition number
    >= 1 of the float32 sum its gradient is (aux_cond) - the deviation is divided by it."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    e = np.abs(got - ref) / np.maximum(np.abs(ref), lr)
    return float(np.max(e if cond is None else e / cond, initial=0.0))


def aux_cond(tail, aux, hyper):
    """Per propensity parameter, gross / |gradient| >= 1 (dla_aux_grad): 1 for the W_l, and for the bias the condition number of the
    sum its gradient is.  The update launch forms that sum in float32 and does not report it, so the float64 Adam step can only be fed
    the terms: a relative error of cond x the float32 rounding of a sum is the yardstick's, not the optimizer's."""
    ga, gross = dla_aux_grad(tail, aux, hyper)
    return np.where(np.abs(ga) > 0, gross / np.where(np.abs(ga) > 0, np.abs(ga), 1.0), 1.0).clip(min=1.0)


def moment_excess(got, ref, old, terms):
    """max |got - ref| / max(|ref|, |old|, terms) over the moments: to be held against MOMENT_RTOL.  Both m = b1 m + (1 - b1) g and
    g = g_raw gs + lam p may cancel; the rounding error of a float32 evaluation is proportional to the terms, not to the result."""
    got, ref, old, terms = (np.asarray(a, np.float64) for a in (got, ref, old, terms))
    if not np.isfinite(got).all():
        return float("inf")
    den = np.maximum(np.maximum(np.maximum(np.abs(ref), np.abs(old)), terms), 1e-30)
    return float(np.max(np.abs(got - ref) / den, initial=0.0))


# ------------------------------------------------------------------------------------------------------------------------
# the shared inputs
# ------------------------------------------------------------------------------------------------------------------------
FLAT_P = (1, 255, 257, 1000)       # one element, one short of a workgroup, one over, four workgroups with a ragged last one
FLAT_ALGOS = ("softmax", "dla", "pairdebias", "pdgd")
CLIPS = (0.0, 0.05)                # no clip; a clip that bites (the raw gradients have magnitude up to 1)
L2S = (0.0, 0.01)
FLAT_L = 7
WARM_T = (1000, 10 ** 5, 2 ** 31)  # single steps from non-zero moments: both corrections far from their t = 1 values, then both 1
TILED_HIDDEN = ([256, 64], [256, 256], [512, 256, 128])
TILED_F, TILED_B, TILED_L = 136, 16, 10


def make_grad(rng, n, zero_mask=None):
    """Gradients that are exactly 0 (a tenth of them, or zero_mask) or have magnitude in [1e-3, 1] (log-uniform), random sign."""
    g = np.exp(rng.uniform(np.log(1e-3), 0.0, size=n)) * rng.choice([-1.0, 1.0], size=n)
    g = np.clip(np.abs(g), 1e-3, 1.0) * np.sign(g)
    if zero_mask is None:
        zero_mask = rng.uniform(size=n) < 0.1
    g[zero_mask] = 0.0
    return g.astype(np.float32), zero_mask


def make_tail(rng, algo, L):
    """A step tail [loss_sum, D, loss2_sum, D2, 2 L per-position sums] with values the algorithm's block-0 duties accept."""
    t = np.zeros(TAIL_FIXED + 2 * L, np.float32)
    t[0], t[1], t[2], t[3] = 3.5, 1.0, 2.25, 2.0
    if algo == "dla":     # d exam / d propensity sums: zero or magnitude in [1e-3, 1], as the gradients - of ONE sign, so that the
        # bias gradient (their ELU'-weighted sum, formed in float32 on the GPU and not reported) cannot cancel to a rounding error
        t[TAIL_FIXED:TAIL_FIXED + L] = np.abs(make_grad(rng, L)[0])
    elif algo == "pairdebias":  # t_plus_loss | t_minus_loss: positive
        t[TAIL_FIXED:] = rng.uniform(0.5, 1.5, size=2 * L)
    return t


def make_aux(rng, algo, L):
    if algo == "dla":
        q = rng.normal(scale=0.3, size=L + 1)
        q[0], q[1] = 0.2 - q[L], -0.3 - q[L]  # both branches of ELU'
        return q.astype(np.float32)
    if algo == "pairdebias":
        return rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32)
    return None


def _case(name, algo, P, L, clip, l2, p0, seed):
    """One case: a fresh run of steps t = 1, 2, 3 (the zero gradients stay where they are, so their v stays 0) and one warm step
    at each of WARM_T from non-zero moments."""
    rng = np.random.RandomState(seed)
    hyper = adam_hyper(algo, max_gradient_norm=clip, l2_loss=l2, propensity_learning_rate=0.02 if algo == "dla" else None)
    g1, zm = make_grad(rng, P)
    fresh = [(t, g1 if t == 1 else make_grad(rng, P, zm)[0], make_tail(rng, algo, L)) for t in (1, 2, 3)]
    nst = state_floats(algo, P, L)
    warm = []
    for t in WARM_T:
        # moments a run of gradients of magnitude 1e-3 .. 1e-1 leaves: v in [1e-6, 1e-2], |m| <= 0.9 sqrt(v)
        v0 = rng.uniform(1e-6, 1e-2, size=P)
        st = np.concatenate([0.9 * np.sqrt(v0) * rng.uniform(-1, 1, size=P), v0])
        if algo == "dla":
            va = rng.uniform(1e-6, 1e-2, size=L + 1)
            st = np.concatenate([st, 0.9 * np.sqrt(va) * rng.uniform(-1, 1, size=L + 1), va])
        assert len(st) == nst
        warm.append((t, make_grad(rng, P)[0], make_tail(rng, algo, L), st.astype(np.float32)))
    return dict(name=name, algo=algo, P=P, L=L, hyper=hyper, p0=np.asarray(p0, np.float32), aux0=make_aux(rng, algo, L),
                zero_mask=zm, fresh=fresh, warm=warm)


@functools.lru_cache(maxsize=None)
def flat_cases():
    out = []
    for P in FLAT_P:
        for algo in FLAT_ALGOS:
            for clip in CLIPS:
                for l2 in L2S:
                    name = "flat-%s-P%d-clip%g-l2%g" % (algo, P, clip, l2)
                    seed = (P * 131 + FLAT_ALGOS.index(algo) * 17 + CLIPS.index(clip) * 5 + L2S.index(l2)) % 2147483629
                    p0 = np.random.RandomState(seed + 1).uniform(-1, 1, size=P)
                    out.append(_case(name, algo, P, FLAT_L, clip, l2, p0, seed))
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def tiled_cases():
    """The three DNNs of test_gpu_edges.py::test_update_kernel_keeps_every_weight_copy_current, parameters as there."""
    from oracle import ultr_oracle as O
    out = []
    for k, hidden in enumerate(TILED_HIDDEN):
        p0 = O.init_params(TILED_F, hidden, seed=9)
        name = "tiled-" + "x".join(str(h) for h in hidden)
        out.append(dict(_case(name, "softmax", len(p0), TILED_L, 0.05 if k == 1 else 0.0, 0.01 if k == 2 else 0.0, p0, 977 + k),
                        hidden=hidden))
    return {c["name"]: c for c in out}


def walk(case, step):
    """Teacher-forced walk of a case with `step` (step64 / step32) against step64: yields (t, got, ref64, state before the step)
    with got / ref64 = (parameters, state, aux) after it; every step starts from the float32 rounding of the YARDSTICK's previous result,
    as the GPU tests start every step from the GPU's own float32 values."""
    h, algo, P, L = case["hyper"], case["algo"], case["P"], case["L"]
    p, st, aux = case["p0"], np.zeros(state_floats(algo, P, L), np.float32), case["aux0"]
    runs = [(t, g, tail, None) for t, g, tail in case["fresh"]] + list(case["warm"])
    for t, g, tail, st_in in runs:
        if st_in is not None:
            p, st, aux = case["p0"], st_in, case["aux0"]
        a = aux if algo == "dla" else None
        ref, got = step64(p, g, st, t, h, tail, a), step(p, g, st, t, h, tail, a)
        yield t, got, ref, st
        p, st = ref[0].astype(np.float32), ref[1].astype(np.float32)
        if algo == "dla":
            aux = ref[2].astype(np.float32)
