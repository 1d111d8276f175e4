"""The list-loss kernels (csrc/ultr_loss.hip) and the step tail's duties in the update launch (csrc/ultr_update.hip:
update_body) restated in float64 numpy, for the tests - a restatement of the KERNELS' contract, not of torch:

    scores [B, L], labels [L, B]; the kernels emit d(loss)/d(scores) x D (the global normaliser D is applied by the update
    launch) and one step tail  [loss_sum, D, loss2_sum, D2, per-position sums (2L)]  per batch.

Every loss function returns a dict with
    tail      [4 + 2L]   the step tail, summed over the lists of the batch
    ds        [B, L]     dscores x D
    ds_abs    [B, L]     per dscores entry, the sum of the absolute values of the terms it is a sum of
    tail_abs  [4 + 2L]   the same for every word of the tail
- the scale a float32 evaluation's rounding and summation-order differences are proportional to (as
oracle.dnn_backward_manual(..., abs_terms=True) gives for the DNN's gradient).  tail_update() / param_update() restate block 0's
per-position duties and the elementwise clip + optimizer step.  The case tables at the end are shared by
tests/test_loss_ref_cpu.py (the float32 oracle holds every bar on them: the inputs are fair) and tests/test_gpu_losses.py."""
import functools

import numpy as np

TAIL_FIXED = 4
SMOOTH = float(np.float32(0.0000001))  # the reference's 1e-7 label smoothing, as the kernels hold it

# ---- the bars of tests/test_gpu_losses.py (all from this project) ---------------------------------------------------------
SCALAR_RTOL = 1e-5   # loss and step scalars: 1e-5 * max(1, |ref|)
TERMS_RTOL = 1e-5    # dscores and per-position sums: |got - ref| <= 1e-5 * (|ref| + sum |terms|)   (test_gpu_edges.py:
#                      test_split_half_weight_gradients_across_a_wide_range_of_dz)
AUX_ATOL = 1e-6      # per-position state after the update (the golden bar, test_gpu_parity.py)
# Parameters and accumulators against param_update() on the SAME float32 gradient: only float32 rounding of a handful of
# operations separates the two.  Measured on the CPU (test_loss_ref_cpu.py::test_oracle_update_error_is_inside_the_measured_figures)
# over every case of hyper_cases(): the float32 oracle's apply_update differs from param_update by at most
PARAM_ERR_MEASURED = 6.2e-8   # max |p' - ref|  (parameters of order 1: half an ulp of the last subtraction)
STATE_ERR_MEASURED = 2.8e-7   # max |s' - ref| / max(ref, 1e-30)
# and the GPU gets 4 x that: a different but equally valid float32 evaluation order (g x gs x coef against (g x coef) of an
# already normalised gradient, lr x (g / d) against (lr x g) / d)
PARAM_ATOL = 4.0 * PARAM_ERR_MEASURED
STATE_RTOL = 4.0 * STATE_ERR_MEASURED
# `aux` after the update with regulation_p = 0 (the ratio t_loss / t_loss[0] is not damped by a root): the float32 oracle's own
# error against tail_update() on the same case, measured by test_loss_ref_cpu.py::test_oracle_step_tail_holds_the_gpu_bars
AUX_P0_ERR_MEASURED = {"pairdebias": 1.1e-7, "lambdarank": 1.0e-7}  # (so the bar stays 1e-6)


def aux_atol(case):
    if case["algo"] in AUX_P0_ERR_MEASURED and float(case["kw"].get("regulation_p", 1.0)) == 0.0:
        return max(AUX_ATOL, 4.0 * AUX_P0_ERR_MEASURED[case["algo"]])
    return AUX_ATOL


def _f8(a):
    return np.asarray(a, np.float64)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _lse(x):
    m = x.max(-1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(-1, keepdims=True))


def _tail(L, head, pos=None, pos2=None):
    t = np.zeros(TAIL_FIXED + 2 * L, np.float64)
    t[:len(head)] = head
    if pos is not None:
        t[TAIL_FIXED:TAIL_FIXED + L] = pos
    if pos2 is not None:
        t[TAIL_FIXED + L:] = pos2
    return t


# ------------------------------------------------------------------------------------------------------------------------
# the five losses
# ------------------------------------------------------------------------------------------------------------------------
def softmax_ce(scores, labels_LB, pw=None, ipw=None):
    """w = (y + 1e-7) p with p = pw[b, l], or (IPW) ipw[min(l, n - 1)] on clicked documents and 0 elsewhere, or 1;
    S_b = sum_l w; loss_sum = sum_b sum_l w (lse_b - s); D = sum_b S_b; dscores x D = softmax(s) S_b - w."""
    s, y = _f8(scores), _f8(labels_LB).T
    B, L = s.shape
    if pw is not None:
        p = _f8(pw)
    elif ipw is not None:
        tab = _f8(np.asarray(ipw, np.float32))
        p = np.where(y > 0, tab[np.minimum(np.arange(L), len(tab) - 1)][None, :], 0.0)
    else:
        p = np.ones_like(s)
    w = (y + SMOOTH) * p
    S = w.sum(1, keepdims=True)
    lse = _lse(s)
    sm = np.exp(s - lse)
    terms = w * (lse - s)
    return dict(tail=_tail(L, [terms.sum(), S.sum()]), ds=sm * S - w, ds_abs=sm * np.abs(S) + np.abs(w),
                tail_abs=_tail(L, [np.abs(terms).sum(), np.abs(w).sum()]))


def _to_prob(x, l2p):
    if l2p == "sigmoid":
        return _sigmoid(x - x.mean(-1, keepdims=True))
    return np.exp(x - _lse(x))


def dla(scores, labels_LB, prop_params, l2p="softmax"):
    """propensity logits pl = ELU(W_l + bias); weights (y + 1e-7) prob[0] / prob[l] with prob = softmax or sigmoid(x - mean) of
    the propensity logits (rank loss) and of the scores (exam loss); both losses are softmax cross entropies.  Tail: rank
    loss_sum, D_rank, exam loss_sum, D_exam, sum_b d exam / d propensity[b, l] x D_exam."""
    s, y, q = _f8(scores), _f8(labels_LB).T, _f8(prop_params)
    B, L = s.shape
    z = q[:L] + q[L]
    pl = np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))[None, :]
    pp, pr = _to_prob(pl, l2p), _to_prob(s, l2p)
    wr = (y + SMOOTH) * (pp[:, :1] / pp)
    we = (y + SMOOTH) * (pr[:, :1] / pr)
    Sr, Se = wr.sum(1, keepdims=True), we.sum(1, keepdims=True)
    lses, lsep = _lse(s), _lse(pl)
    sms, smp = np.exp(s - lses), np.exp(pl - lsep)
    tr, te = wr * (lses - s), we * (lsep - pl)
    return dict(tail=_tail(L, [tr.sum(), Sr.sum(), te.sum(), Se.sum()], (smp * Se - we).sum(0)),
                ds=sms * Sr - wr, ds_abs=sms * Sr + wr,
                tail_abs=_tail(L, [np.abs(tr).sum(), Sr.sum(), np.abs(te).sum(), Se.sum()], (smp * Se + we).sum(0)))


def pairdebias(scores, labels_LB, t_plus, t_minus, batch_total=None):
    """Per list and ordered pair (i, j) with c_i > c_j:  PL_ij += B min(1, c_i - c_j) softplus(s_j - s_i)  (B: the reference's
    [B] x [B, 1] broadcast);  t_plus_loss[i] = sum_j PL_ij / t-_j,  t_minus_loss[j] = sum_i PL_ij / t+_i,
    loss = sum PL_ij / t+_i / t-_j.  D is unused (one per list)."""
    s, c, tp, tm = _f8(scores), _f8(labels_LB).T, _f8(t_plus), _f8(t_minus)
    B, L = s.shape
    bs = float(B if batch_total is None else batch_total)
    m = np.minimum(1.0, np.maximum(c[:, :, None] - c[:, None, :], 0.0))  # [b, i, j]
    x = s[:, None, :] - s[:, :, None]                                     # s_j - s_i
    PL = bs * m * _softplus(x)
    gw = bs * m * _sigmoid(x) / tp[None, :, None] / tm[None, None, :]
    tpl = (PL / tm[None, None, :]).sum((0, 2))
    tml = (PL / tp[None, :, None]).sum((0, 1))
    loss = (PL / tp[None, :, None] / tm[None, None, :]).sum()
    return dict(tail=_tail(L, [loss, float(B)], tpl, tml), ds=gw.sum(1) - gw.sum(2), ds_abs=gw.sum(1) + gw.sum(2),
                tail_abs=_tail(L, [loss, float(B)], tpl, tml))


def stable_order(scores):
    """Descending by score, ties broken by original index (what lambdarank_kernel's rank-by-counting produces)."""
    return np.argsort(-_f8(scores), axis=1, kind="stable")


def lambdarank(scores, labels_LB, t_plus, t_minus, sigma=1.0):
    """On the list sorted by score (stable): delta_rc = |g_r - g_c| |d_r - d_c| with g = 2^y - 1, d = 1 / log2(rank + 2);
    target (1 + clamp(y_r - y_c, -1, 1)) / 2; x_rc = sigmoid(sigma (s_r - s_c)); PL_rc = sum_b delta x BCE-with-logits(x, target)
    (applied to the PROBABILITY x - the reference's quirk).  t_plus_loss[r] = sum_c PL_rc / t-_c, t_minus_loss[r] = sum_c PL_cr /
    t+_c, loss = sum safe_div(PL_rc, t+_r t-_c); everything x IDCG: D = sum_b ideal DCG with natural-log discounts."""
    s, y, tp, tm = _f8(scores), _f8(labels_LB).T, _f8(t_plus), _f8(t_minus)
    B, L = s.shape
    order = stable_order(s)
    ps, ls = np.take_along_axis(s, order, 1), np.take_along_axis(y, order, 1)
    g = np.exp2(ls) - 1.0
    d = 1.0 / np.log2(np.arange(L) + 2.0)
    delta = np.abs(g[:, :, None] - g[:, None, :]) * np.abs(d[:, None] - d[None, :])[None]
    pb = 0.5 * (1.0 + np.clip(ls[:, :, None] - ls[:, None, :], -1.0, 1.0))
    z = sigma * (ps[:, :, None] - ps[:, None, :])
    x, xc = _sigmoid(z), _sigmoid(-z)
    l = delta * (x - x * pb + np.log1p(np.exp(-x)))
    PL = l.sum(0)
    ok = (tp[:, None] * tm[None, :]) != 0.0
    den = np.where(ok, tp[:, None] * tm[None, :], 1.0)
    tpl = (PL / tm[None, :]).sum(1)
    tml = (PL / tp[:, None]).sum(0)
    loss = np.where(ok, PL / den, 0.0).sum()
    ideal = -np.sort(-y, axis=1)
    idcg = ((np.exp2(ideal) - 1.0) / np.log(np.arange(L) + 2.0)[None, :]).sum()
    A = np.where(ok[None], delta * (_sigmoid(x) - pb) * (sigma * x * xc) / den[None], 0.0)  # d loss / d s_r through PL_rc
    dsort, dsort_abs = A.sum(2) - A.sum(1), np.abs(A).sum(2) + np.abs(A).sum(1)
    ds, ds_abs = np.zeros_like(s), np.zeros_like(s)
    np.put_along_axis(ds, order, dsort, 1)
    np.put_along_axis(ds_abs, order, dsort_abs, 1)
    return dict(tail=_tail(L, [loss, idcg], tpl, tml), ds=ds, ds_abs=ds_abs, tail_abs=_tail(L, [loss, idcg], tpl, tml), order=order)


def regem(scores, labels_LB, propensity, uniforms):
    """E-step from the current scores and propensity, pseudo-labels y = ceil(P(r = 1) - u), loss_sum = sum BCE-with-logits(s, y),
    D = B L, dscores x D = sigmoid(s) - y, per-position sums of c + (1 - c) P(e = 1, r = 0 | c = 0)."""
    s, c, pr, u = _f8(scores), _f8(labels_LB).T, _f8(propensity)[None, :], _f8(uniforms)
    B, L = s.shape
    gamma, gammac = _sigmoid(s), _sigmoid(-s)
    den = 1.0 - pr * gamma
    p_e1_r0 = pr * gammac / den
    p_r1 = c + (1.0 - c) * ((1.0 - pr) * gamma / den)
    y = np.ceil(p_r1 - u)
    bce = np.maximum(s, 0.0) - s * y + np.log1p(np.exp(-np.abs(s)))
    pos = c + (1.0 - c) * p_e1_r0
    return dict(tail=_tail(L, [bce.sum(), float(B * L)], pos.sum(0)), ds=gamma - y, ds_abs=gamma + np.abs(y),
                tail_abs=_tail(L, [np.abs(bce).sum(), float(B * L)], np.abs(pos).sum(0)), pseudo=y, p_r1=p_r1)


# ------------------------------------------------------------------------------------------------------------------------
# block 0 of the update launch and the elementwise step
# ------------------------------------------------------------------------------------------------------------------------
HYPER = dict(optimizer="ada", learning_rate=0.05, max_gradient_norm=5.0, ranker_loss_weight=1.0, propensity_learning_rate=None,
             em_step_size=0.05, regulation_p=1.0, l2_loss=0.0, adagrad_eps=1e-10)


def hyper_of(algo, **kw):
    """The update descriptor's hyper-parameters as the kernel holds them: float32 values (engine.StepEngine's defaults)."""
    h = dict(HYPER)
    h.update({k: v for k, v in kw.items() if k in HYPER})
    if h["propensity_learning_rate"] is None or h["propensity_learning_rate"] < 0:
        h["propensity_learning_rate"] = h["learning_rate"]
    h = {k: (v if k == "optimizer" else float(np.float32(v))) for k, v in h.items()}
    h["algo"] = algo
    return h


def _opt_step(p, g, s_old, opt, stateless, lr, eps):
    """(p', s') - torch.optim.Adagrad with lr_decay 0 (s += g g; p -= lr g / (sqrt(s) + eps)) or SGD."""
    if opt == "sgd":
        return p - lr * g, s_old
    s = (0.0 if stateless else s_old) + g * g
    return p - lr * (g / (np.sqrt(s) + eps)), s


def step_scalars(tail, ss, hyper, l2_sums=None):
    """gs (what turns the raw gradient into the gradient), loss, norm, coef, D, rank_loss, exam_loss, lam (the L2 factor) from the
    tail, the sum of squares of the RAW gradient and (l2_loss > 0) l2_sums = (sum p^2, sum g_raw p)."""
    algo = hyper["algo"]
    loss_sum, D, loss2, D2 = [float(v) for v in tail[:4]]
    rank_loss = exam_loss = 0.0
    if algo == "dla":
        rank_loss, exam_loss = loss_sum / D, loss2 / D2
        gs = hyper["ranker_loss_weight"] / D
        loss = exam_loss + hyper["ranker_loss_weight"] * rank_loss
    elif algo == "pairdebias":
        gs, loss = 1.0, loss_sum
    else:  # softmax, lambdarank, regem
        gs, loss = 1.0 / D, loss_sum / D
    norm = abs(gs) * np.sqrt(ss)
    lam, clip = 0.0, hyper["max_gradient_norm"] > 0
    if hyper["l2_loss"] > 0:
        sp2, sgp = l2_sums
        if algo == "dla":  # inside rank_loss, both clips stay active
            lam = hyper["ranker_loss_weight"] * hyper["l2_loss"]
            rank_loss += hyper["l2_loss"] * 0.5 * sp2
            loss = exam_loss + hyper["ranker_loss_weight"] * rank_loss
        else:              # the reference hands clip_grad_norm_ an exhausted generator: nothing is clipped
            lam = hyper["l2_loss"]
            loss += hyper["l2_loss"] * 0.5 * sp2
            clip = False
        norm = np.sqrt(max(gs * gs * ss + 2.0 * gs * lam * sgp + lam * lam * sp2, 0.0))
    coef = min(1.0, hyper["max_gradient_norm"] / (norm + 1e-6)) if clip else 1.0
    return dict(gs=gs, loss=loss, norm=norm, coef=coef, D=D, rank_loss=rank_loss, exam_loss=exam_loss, lam=lam)


def tail_update(algo, tail, aux, hyper, ss=0.0, l2_sums=None):
    """Block 0's duties: (new aux, dict(loss, norm, coef, D, rank_loss, exam_loss, pnorm))."""
    assert algo == hyper["algo"]
    tail = _f8(tail)
    L = (len(tail) - TAIL_FIXED) // 2
    sc = step_scalars(tail, ss, hyper, l2_sums)
    pnorm = 0.0
    new = None if aux is None else _f8(aux).copy()
    a = hyper["em_step_size"]
    if algo == "dla":
        bias = new[L]
        z = new[:L] + bias
        g = tail[TAIL_FIXED:TAIL_FIXED + L] / tail[3] * np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))  # ELU' chain
        gsum = g.sum()
        pnorm = float(np.sqrt((g * g).sum() + gsum * gsum))
        pc = min(1.0, hyper["max_gradient_norm"] / (pnorm + 1e-6)) if hyper["max_gradient_norm"] > 0 else 1.0
        lr, eps = hyper["propensity_learning_rate"], hyper["adagrad_eps"]
        new[:L] = _opt_step(new[:L], g * pc, 0.0, hyper["optimizer"], True, lr, eps)[0]
        new[L] = _opt_step(bias, gsum * pc, 0.0, hyper["optimizer"], True, lr, eps)[0]
    elif algo in ("pairdebias", "lambdarank"):
        ex = 1.0 / (hyper["regulation_p"] + 1.0)
        for h in range(2):
            num = tail[TAIL_FIXED + h * L:TAIL_FIXED + (h + 1) * L]
            ratio = np.zeros(L) if (algo == "lambdarank" and num[0] == 0.0) else num / num[0]
            new[h * L:(h + 1) * L] = (1.0 - a) * new[h * L:(h + 1) * L] + a * np.power(ratio, ex)
    elif algo == "regem":
        nb = tail[1] / L  # lists in the batch
        new[:L] = (1.0 - a) * new[:L] + a * (tail[TAIL_FIXED:TAIL_FIXED + L] / nb)
    out = {k: sc[k] for k in ("loss", "norm", "coef", "D", "rank_loss", "exam_loss")}
    out["pnorm"] = pnorm
    return new, out


def l2_sums_of(p, g_raw):
    p, g = _f8(p), _f8(g_raw)
    return float((p * p).sum()), float((g * p).sum())


def param_update(p, g_raw, state, ss, hyper, tail):
    """Clip + Adagrad / SGD of every parameter from the RAW gradient (x D), its sum of squares and the tail:
    g = g_raw gs (+ lam p), x coef; DLA's optimizer is stateless.  Returns (p', s')."""
    p, g_raw = _f8(p), _f8(g_raw)
    sc = step_scalars(_f8(tail), float(ss), hyper, l2_sums_of(p, g_raw) if hyper["l2_loss"] > 0 else None)
    g = g_raw * sc["gs"]
    if sc["lam"] != 0.0:
        g = g + sc["lam"] * p
    g = g * sc["coef"]
    stateless = hyper["algo"] == "dla"
    s_old = np.zeros_like(p) if state is None else _f8(state)
    pn, sn = _opt_step(p, g, s_old, hyper["optimizer"], stateless, hyper["learning_rate"], hyper["adagrad_eps"])
    return pn, (s_old if (stateless or hyper["optimizer"] == "sgd") else sn)


# ------------------------------------------------------------------------------------------------------------------------
# the shared case tables
# ------------------------------------------------------------------------------------------------------------------------
ALGOS = ("softmax", "dla", "pairdebias", "lambdarank", "regem")
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 255, 256)   # lane (64) and slice (LOSS_JW = 16) boundaries, the 256 cap
SCALE_LENGTHS = (17, 65, 256)
# Scores x 8: pair gaps reach about +-50, sigmoids and softplus saturate, nothing overflows in float32.  (Per algorithm: the largest
# of 8, 4, 2 at which the float32 oracle itself holds the bars, test_loss_ref_cpu.py::test_oracle_losses_hold_the_gpu_bars.)
# LambdaRank runs at 4: at 8 and L = 256 only neighbours in rank are unsaturated, their weight |d_r - d_c| is a difference of float32
# discounts 1 / log2(rank + 2) that agree to four digits around rank 200, and the float32 oracle itself is 3.1e-5 of the terms away from
# float64 there (5.6e-6 at 4).
SCORE_SCALE = {"softmax": 8.0, "dla": 8.0, "pairdebias": 8.0, "lambdarank": 4.0, "regem": 8.0}
TOY_F, TOY_HIDDEN = 8, [4]


def _seed(*key):
    h = 0
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % 2147483629
    return h


def make_case(name, algo, B, L, scale=1.0, labels="default", tie=0, net=False, state="zero", aux_scale=1.0, **kw):
    """One input set.  labels: "default" (binary clicks at rate 0.3, position 0 clicked; LambdaRank: grades 0..4), "graded" (0..4),
    "fractional" ({0, 0.5, 1}), "sparse" (list 0 without a click, list 1 with a single click), "flat" (LambdaRank: list 0 all
    equal).  tie: the last `tie` documents of every list share one score, with labels that differ inside the tie.  net: also
    the toy net's inputs (features, docids, parameters, Adagrad state "zero" or "rand" = 0.01 x uniform)."""
    rng = np.random.RandomState(_seed(name))
    scores = (scale * rng.normal(size=(B, L))).astype(np.float32)
    if tie:
        scores[:, L - tie:] = np.float32(0.125)
    y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    y[0, :] = 1.0
    if algo == "lambdarank" or labels == "graded":
        y = rng.randint(0, 5, size=(L, B)).astype(np.float32)
        y[0, :] = np.maximum(y[0, :], 1.0)
    if labels == "fractional":
        y = (rng.randint(0, 3, size=(L, B)) * 0.5).astype(np.float32)
        y[0, :] = 1.0
    if labels == "sparse":
        y[:, 0] = 0.0
        y[:, 1] = 0.0
        y[min(5, L - 1), 1] = 1.0
    if labels == "flat":
        y[:, 0] = 2.0
    if tie:
        blk = np.arange(tie)
        y[L - tie:, :] = ((blk % 5) if (algo == "lambdarank") else (blk % 2)).astype(np.float32)[:, None]
    case = dict(name=name, algo=algo, B=B, L=L, scores=scores, labels=y, aux=None, ipw=None, uniforms=None, kw=dict(kw), tie=tie)
    if algo == "softmax":
        case["ipw"] = None if labels == "sparse" else rng.uniform(1, 10, size=40).astype(np.float32)
    elif algo == "dla":
        q = rng.normal(scale=0.3, size=L + 1)
        q[0], q[min(1, L - 1)] = 0.2 - q[L], -0.3 - q[L]  # both branches of ELU' among the logits (L = 1: the negative one)
        case["aux"] = (aux_scale * q).astype(np.float32)
    elif algo in ("pairdebias", "lambdarank"):
        case["aux"] = rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32)
    elif algo == "regem":
        prop = rng.uniform(0.1, 0.9, size=L)
        prop[:3] = [0.95, 0.5, 0.05][:min(3, L)]
        case["aux"] = prop.astype(np.float32)
        # uniforms away from the pseudo-label's threshold: y = ceil(P(r = 1) - u) is discrete, and a float32 P within rounding
        # of u would make the label itself a matter of evaluation order
        u = rng.uniform(size=(B, L)).astype(np.float32)
        p_r1 = regem(scores, y, case["aux"], u)["p_r1"]
        near = np.abs(p_r1 - u) < 1e-4
        u[near] = np.where(p_r1[near] > 0.5, p_r1[near] - 0.01, p_r1[near] + 0.01).astype(np.float32)
        case["uniforms"] = u
    if net and algo == "pairdebias":
        # the EM step divides by t_minus_loss[0] with a plain "/": a position 0 that every list clicked never loses a pair and the
        # reference's own ratio is 0 / 0
        y[0, 0], y[1, 0] = 0.0, 1.0
        case["labels"] = y
    if net:
        from oracle import ultr_oracle as O
        case["feats"] = rng.uniform(-1, 1, size=(B * L, TOY_F)).astype(np.float32)
        case["ids"] = rng.permutation(B * L).astype(np.int32).reshape(L, B)
        params = O.init_params(TOY_F, TOY_HIDDEN, seed=_seed(name) % 1000)
        params += rng.uniform(-0.2, 0.2, size=params.shape).astype(np.float32)
        case["params"] = params
        case["state"] = (0.01 * rng.uniform(size=params.shape)).astype(np.float32) if state == "rand" else np.zeros_like(params)
    return case


@functools.lru_cache(maxsize=None)
def loss_cases():
    """The loss-kernel cases: {name: case}."""
    out = []
    for algo in ALGOS:
        for L in LENGTHS:
            out.append(make_case("len-%s-L%d" % (algo, L), algo, 3, L))
        for L in (65, 129, 256):  # DLA with logits_to_prob = sigmoid beyond 64 positions
            if algo == "dla":
                out.append(make_case("len-dla-sigmoid-L%d" % L, algo, 3, L, logits_to_prob="sigmoid"))
        for L in SCALE_LENGTHS:
            out.append(make_case("scale-%s-L%d" % (algo, L), algo, 3, L, scale=SCORE_SCALE[algo]))
    out.append(make_case("labels-pairdebias-graded", "pairdebias", 3, 17, labels="graded"))
    out.append(make_case("labels-pairdebias-fractional", "pairdebias", 3, 17, labels="fractional"))
    for algo in ("softmax", "dla", "pairdebias", "regem"):
        out.append(make_case("labels-%s-sparse" % algo, algo, 3, 17, labels="sparse"))
    out.append(make_case("labels-lambdarank-flat", "lambdarank", 3, 17, labels="flat"))
    for algo in ("lambdarank", "pairdebias"):
        for L in (20, 70):
            for k in (1, 5, L - 1):
                out.append(make_case("tie-%s-L%d-k%d" % (algo, L, k), algo, 3, L, tie=k))
    # the longest lists the pair-walk kernels accept (160 KiB of LDS, tests/test_loss_layout_cpu.py): the last word of the layout
    out.append(make_case("edge-pairdebias-L585", "pairdebias", 2, 585))
    out.append(make_case("edge-lambdarank-L531", "lambdarank", 2, 531))
    return {c["name"]: c for c in out}


HB, HL = 5, 19  # the step cases: more than one list, a length that is no multiple of the slice count


def _hc(tag, algo, **kw):
    return make_case("step-%s-%s" % (algo, tag), algo, HB, HL, net=True, **kw)


@functools.lru_cache(maxsize=None)
def hyper_cases():
    """loss -> backward -> update on the toy net with one hyper-parameter off its default: {name: case}."""
    out = [_hc("sigma0.5", "lambdarank", sigma=0.5, state="rand"), _hc("sigma2", "lambdarank", sigma=2.0, state="rand")]
    for algo in ("pairdebias", "lambdarank"):
        for p in (0.0, 1.0, 2.0):
            out.append(_hc("p%g" % p, algo, regulation_p=p, state="rand"))
    for algo in ("pairdebias", "lambdarank", "regem"):
        out.append(_hc("em0.2", algo, em_step_size=0.2, state="rand"))
    out.append(_hc("rlw0.3-plr0.02", "dla", ranker_loss_weight=0.3, propensity_learning_rate=0.02))
    out.append(_hc("rlw0.3", "dla", ranker_loss_weight=0.3))
    for algo in ALGOS:
        for mg in (0.0, 0.01, 5.0):  # no clip, a clip that bites (coef < 1; DLA: pc < 1 too), the default
            out.append(_hc("clip%g" % mg, algo, max_gradient_norm=mg, state="rand"))
        out.append(_hc("zero-state", algo))
    # DLA's own clip: Adagrad's first step is sign-like, so pc < 1 only shows under SGD; the propensity logits x 3 make the
    # propensity gradient larger than the bound
    out.append(_hc("pc", "dla", optimizer="sgd", max_gradient_norm=0.05, aux_scale=3.0))
    for algo in ("softmax", "pairdebias", "regem"):
        out.append(_hc("sgd", algo, optimizer="sgd"))
        out.append(_hc("sgd-clip0.01", algo, optimizer="sgd", max_gradient_norm=0.01))
    for algo in ("softmax", "dla", "pairdebias", "regem"):
        out.append(_hc("l2", algo, l2_loss=1.0, state="rand"))
    return {c["name"]: c for c in out}


MANY = [("dla", 1100), ("pairdebias", 1100), ("lambdarank", 1100), ("regem", 1100), ("pairdebias", 1024), ("pairdebias", 1025)]
MANY_L = 33  # a 70-word tail: two 64-lane passes of the fold; more than 1024 lists: the two-level fold


@functools.lru_cache(maxsize=None)
def many_case(algo, B):
    return make_case("many-%s-B%d" % (algo, B), algo, B, MANY_L, net=True, state="rand")


_REF = {}


def reference(case):
    """The restatement on a case, computed once per process."""
    r = _REF.get(case["name"])
    if r is None:
        a, s, y = case["algo"], case["scores"], case["labels"]
        L = case["L"]
        if a == "softmax":
            r = softmax_ce(s, y, ipw=case["ipw"])
        elif a == "dla":
            r = dla(s, y, case["aux"], case["kw"].get("logits_to_prob", "softmax"))
        elif a == "pairdebias":
            r = pairdebias(s, y, case["aux"][:L], case["aux"][L:])
        elif a == "lambdarank":
            r = lambdarank(s, y, case["aux"][:L], case["aux"][L:], float(np.float32(case["kw"].get("sigma", 1.0))))
        else:
            r = regem(s, y, case["aux"], case["uniforms"])
        _REF[case["name"]] = r
    return r


def terms_excess(got, ref, terms):
    """max of |got - ref| / (|ref| + sum |terms|) over the entries (0 where both are 0): to be held against TERMS_RTOL."""
    got, ref, terms = _f8(got), _f8(ref), _f8(terms)
    den = np.abs(ref) + terms
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
