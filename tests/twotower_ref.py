"""The float64 twin of the TwoTower learning algorithm (csrc/ultr_twotower.hip, the ULTR_ALGO_TWOTOWER branch of csrc/ultr_update.hip,
learning_algorithm/two_tower.py), for the tests.  The loss is written from its definition in torch float64, the gradients are
autograd's, the clip is torch.nn.utils.clip_grad_norm_ per tower and the optimizers are torch.optim.Adagrad / SGD / Adam on two
parameter groups (the ranker at learning_rate, the observation tower theta at propensity_learning_rate) with persistent state.

    scores s [B, L], theta [L], labels [L, B] (position-major), click c = min(label, 1)
    product:  p = sigmoid(s) sigmoid(theta_l);   sum:  p = sigmoid(s + theta_l)
    element loss  l = -c log p - (1 - c) log(1 - p);   loss = (1 / B) sum_b sum_l l;   D = B (one per list)
    docids [L, B] with n_docs: a PAD (id < 0 or >= n_docs) contributes nothing to the loss, to dscores, to theta's gradient

loss_parts() returns what the kernel emits - dscores x D, the step tail [sum l, B, 0, 0, sum_b dl/dtheta_l, 0 ...] - with, per entry,
the sum of the absolute values of the terms it is a sum of (loss_ref.terms_excess's scale).  Twin runs whole steps.

The bars are tests/loss_ref.py's (TERMS_RTOL, SCALAR_RTOL, AUX_ATOL, PARAM_ATOL, STATE_RTOL) and, for Adam, tests/adam_ref.py's, unchanged.
excess() is loss_ref.terms_excess on every entry a float32 can hold to a relative bar at all.  Exempt are only the entries whose
reference AND term scale lie below FLT_MIN, the smallest normal float32 (saturated towers: sigmoid(-50) sigmoid(-50) = e^-100): a
float32 below FLT_MIN has no relative precision and hardware may flush it to zero, so such an entry is asked to be below FLT_MIN
itself, nothing else."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_ref as R

TAIL_FIXED = R.TAIL_FIXED
FLT_MIN = float(np.finfo(np.float32).tiny)
LN9 = float(np.log(9.0))


def excess(got, ref, terms):
    """loss_ref.terms_excess over the entries with |ref| + terms >= FLT_MIN; an entry below that must itself be below FLT_MIN in
    magnitude (inf otherwise)."""
    got, ref, terms = (np.asarray(a, np.float64).ravel() for a in (got, ref, np.broadcast_to(np.asarray(terms, np.float64), np.shape(ref))))
    tiny = (np.abs(ref) + terms) < FLT_MIN
    if not np.isfinite(got).all() or (np.abs(got[tiny]) >= FLT_MIN).any():
        return float("inf")
    return R.terms_excess(got[~tiny], ref[~tiny], terms[~tiny])


def _t(a):
    return a.detach().clone().double() if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a, np.float64))


def live_mask(docids_LB, n_docs, B, L):
    """[B, L] bool: the position holds a document.  docids None: every position counts."""
    if docids_LB is None:
        return torch.ones(B, L, dtype=torch.bool)
    ids = torch.as_tensor(np.asarray(docids_LB, np.int64)).t()
    return (ids >= 0) & (ids < int(n_docs))


def clicks_BL(labels_LB):
    return torch.clamp(_t(labels_LB).t(), max=1.0)


def element_loss(s, theta, c, combination):
    """[B, L] element losses from the definition, evaluated without cancellation (float64 torch, differentiable in s and theta)."""
    th = theta.view(1, -1)
    if combination == "sum":
        z = s + th
        return -c * F.logsigmoid(z) - (1.0 - c) * F.logsigmoid(-z)
    assert combination == "product"
    log_p = F.logsigmoid(s) + F.logsigmoid(th)
    p = torch.exp(log_p)
    small = p < 0.5
    # 1 - p = sigmoid(-s) + sigmoid(s) sigmoid(-theta): a sum of positives, formed in the log domain
    log_q = torch.logaddexp(F.logsigmoid(-s), F.logsigmoid(s) + F.logsigmoid(-th))
    log_1mp = torch.where(small, torch.log1p(-torch.where(small, p, torch.zeros_like(p))), log_q)
    return -c * log_p - (1.0 - c) * log_1mp


def naive_element_loss(s, theta, c, combination):
    """The same from the textbook expression (exact to 1e-9 only while 1 - p keeps its digits: |s|, |theta| <= 15)."""
    th = theta.view(1, -1)
    p = torch.sigmoid(s + th) if combination == "sum" else torch.sigmoid(s) * torch.sigmoid(th)
    return -c * torch.log(p) - (1.0 - c) * torch.log(1.0 - p)


def closed_form_grads(s, theta, c, combination):
    """(dl/ds, dl/dtheta per element, |terms| of each) from the closed forms of DESIGN.md section 4c."""
    th = theta.view(1, -1).expand_as(s)
    if combination == "sum":
        g = torch.sigmoid(s + th) - c
        a = torch.sigmoid(s + th) + c.abs()
        return g, g, a, a
    log_p = F.logsigmoid(s) + F.logsigmoid(th)
    log_q = torch.logaddexp(F.logsigmoid(-s), F.logsigmoid(s) + F.logsigmoid(-th))
    pq = (1.0 - c) * torch.exp(log_p - log_q)
    ns, nt = torch.sigmoid(-s), torch.sigmoid(-th)
    return ns * (pq - c), nt * (pq - c), ns * (pq + c.abs()), nt * (pq + c.abs())


def loss_parts(scores, labels_LB, theta, combination="product", docids_LB=None, n_docs=None):
    """What ultr_twotower_loss emits, in float64: dict(tail, ds, ds_abs, tail_abs, loss).  Gradients by autograd."""
    s = _t(scores).requires_grad_(True)
    th = _t(theta).requires_grad_(True)
    B, L = s.shape
    c = clicks_BL(labels_LB)
    live = live_mask(docids_LB, n_docs, B, L)
    el = torch.where(live, element_loss(s, th, c, combination), torch.zeros_like(s))
    total = el.sum()
    total.backward()
    with torch.no_grad():
        if combination == "sum":
            z = s + th.view(1, -1)
            el_abs = (c * F.logsigmoid(z)).abs() + ((1.0 - c) * F.logsigmoid(-z)).abs()
        else:
            el_abs = el.abs()  # both terms of an element are >= 0
        _, _, a_s, a_t = closed_form_grads(s, th, c, combination)
        a_s, a_t, el_abs = [torch.where(live, v, torch.zeros_like(v)) for v in (a_s, a_t, el_abs)]
    tail = np.zeros(TAIL_FIXED + 2 * L)
    tail_abs = np.zeros(TAIL_FIXED + 2 * L)
    total = total.detach()
    tail[0], tail[1] = float(total), float(B)
    tail[TAIL_FIXED:TAIL_FIXED + L] = th.grad.numpy()
    tail_abs[0], tail_abs[1] = float(el_abs.sum()), float(B)
    tail_abs[TAIL_FIXED:TAIL_FIXED + L] = a_t.sum(0).numpy()
    return dict(tail=tail, ds=s.grad.numpy(), ds_abs=a_s.numpy(), tail_abs=tail_abs, loss=float(total) / B, live=live.numpy())


# ------------------------------------------------------------------------------------------------------------------------
# the kernel's formulas restated in numpy float32 (csrc/ultr_twotower.hip: tower_of, twotower_product, twotower_sum)
# ------------------------------------------------------------------------------------------------------------------------
def kernel32(s, theta, c, combination):
    """(loss, dl/ds, dl/dtheta) per element in float32 arithmetic, operation for operation as the kernel."""
    f = np.float32
    s, th, c = np.asarray(s, f), np.asarray(theta, f), np.asarray(c, f)
    one, zero = f(1.0), f(0.0)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if combination == "sum":
            z = s + th
            e = np.exp(-np.abs(z))
            r = one / (one + e)
            loss = np.maximum(z, zero) - z * c + np.log1p(e)
            g = np.where(z >= 0, r, e * r) - c
            return loss.astype(f), g.astype(f), g.astype(f)

        def tower(x, t):
            e = np.exp(-np.abs(x))
            r = one / (one + e)
            sig = np.where(x >= 0, r, e * r)
            nsig = np.where(x >= 0, e * r, r)
            nsig_t = np.where(x > 0, np.exp(t - x) * r, r)
            return sig, nsig_t, nsig, np.minimum(x, zero) - np.log1p(e)

        t = np.maximum(zero, np.minimum(s, th))
        a_sig, a_nt, a_n, a_log = tower(s, t)
        b_sig, b_nt, b_n, b_log = tower(th, t)
        p = a_sig * b_sig
        q = a_nt + a_sig * b_nt
        log_p = a_log + b_log
        log_1mp = np.where(p < f(0.5), np.log1p(-p), np.log(q) - t)
        pq = np.where(c < one, (one - c) * (p / q), zero)
        loss = np.where(c > zero, -c * log_p, zero) + np.where(c < one, -(one - c) * log_1mp, zero)
        return loss.astype(f), (a_nt * pq - a_n * c).astype(f), (b_nt * pq - b_n * c).astype(f)


# ------------------------------------------------------------------------------------------------------------------------
# whole steps
# ------------------------------------------------------------------------------------------------------------------------
HYPER = dict(optimizer="ada", learning_rate=0.05, max_gradient_norm=5.0, l2_loss=0.0, propensity_learning_rate=-1.0,
             tower_combination="product", mask_padding=True)


def hyper_of(**kw):
    """The hyper-parameters as the update descriptor holds them: float32 values."""
    h = dict(HYPER)
    h.update(kw)
    if h["propensity_learning_rate"] is None or h["propensity_learning_rate"] < 0:
        h["propensity_learning_rate"] = h["learning_rate"]
    for k in ("learning_rate", "max_gradient_norm", "l2_loss", "propensity_learning_rate"):
        h[k] = float(np.float32(h[k]))
    return h


def theta_init(combination, L):
    return np.full(L, LN9 if combination == "product" else 0.0, np.float32)


def state_floats(optimizer, P, L):
    return {"sgd": 0, "ada": P + L, "adam": 2 * P + 2 * L}[optimizer]


class Twin:
    """Both towers as float64 leaves under ONE torch optimizer with two parameter groups.

    params: the ranker's parameter tensors in the order of the flat vector; scores_fn() -> [B, L] from them (None: the scores are
    handed to step(), which then needs the ranker's gradient forced).  load() puts the towers and the optimizer state where a device
    run stands - parameters, theta, the state vector in ultr_opt_state_floats' layout, the number of steps taken - so that a step can
    be checked from the very inputs the GPU had (a rounding of an earlier step then cannot pass for an error of this one, nor hide one)."""

    def __init__(self, params, theta, hyper, scores_fn=None):
        self.h = hyper
        self.params = [p.detach().clone().double().requires_grad_(True) for p in params]
        self.theta = _t(theta).requires_grad_(True)
        self.scores_fn = scores_fn
        groups = [dict(params=self.params, lr=hyper["learning_rate"]), dict(params=[self.theta], lr=hyper["propensity_learning_rate"])]
        opt = hyper["optimizer"]
        if opt == "sgd":
            self.opt = torch.optim.SGD(groups, lr=hyper["learning_rate"])
        elif opt == "adam":
            self.opt = torch.optim.Adam(groups, lr=hyper["learning_rate"])  # betas (0.9, 0.999), eps 1e-8, no weight decay
            for p in self.params + [self.theta]:
                self.opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
        else:
            self.opt = torch.optim.Adagrad(groups, lr=hyper["learning_rate"])  # eps 1e-10, accumulators from 0
        self.P = sum(p.numel() for p in self.params)
        self.L = self.theta.numel()

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.params]).numpy()

    def _split(self, flat):
        flat, out, o = _t(flat), [], 0
        for p in self.params:
            out.append(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        return out

    def state(self):
        """The optimizer state in the device layout (ultr_opt_state_floats)."""
        opt, ps = self.h["optimizer"], self.params + [self.theta]
        if opt == "sgd":
            return np.zeros(0)
        if opt == "ada":
            return torch.cat([self.opt.state[p]["sum"].reshape(-1) for p in ps]).numpy()
        m = [self.opt.state[p]["exp_avg"].reshape(-1) for p in ps]
        v = [self.opt.state[p]["exp_avg_sq"].reshape(-1) for p in ps]
        return torch.cat(m[:-1] + v[:-1] + [m[-1], v[-1]]).numpy()

    def load(self, flat_params, theta, state, steps_taken):
        P, L, opt = self.P, self.L, self.h["optimizer"]
        with torch.no_grad():
            for p, v in zip(self.params, self._split(flat_params)):
                p.copy_(v)
            self.theta.copy_(_t(theta))
            ps = self.params + [self.theta]
            if opt == "ada":
                st = _t(state)
                for p, v in zip(self.params, self._split(st[:P])):
                    self.opt.state[p]["sum"].copy_(v)
                self.opt.state[self.theta]["sum"].copy_(st[P:P + L])
            elif opt == "adam":
                st = _t(state)
                for p, m, v in zip(self.params, self._split(st[:P]), self._split(st[P:2 * P])):
                    self.opt.state[p]["exp_avg"].copy_(m)
                    self.opt.state[p]["exp_avg_sq"].copy_(v)
                self.opt.state[self.theta]["exp_avg"].copy_(st[2 * P:2 * P + L])
                self.opt.state[self.theta]["exp_avg_sq"].copy_(st[2 * P + L:2 * P + 2 * L])
            if opt != "sgd":
                for p in ps:
                    self.opt.state[p]["step"].fill_(float(steps_taken))

    def step(self, labels_LB, docids_LB=None, n_docs=None, scores=None, force_grad=None, force_theta_grad=None):
        """One training step.  Returns dict(loss, norm, coef, D, pnorm, pcoef, scores, grad (the ranker's, flat, before the clip and
        without the L2 term), theta_grad).  force_grad / force_theta_grad: take these (float32, from the device) as the data
        gradients instead of autograd's - the L2 term, the clips and the optimizers still run here."""
        h = self.h
        self.opt.zero_grad(set_to_none=True)
        s = self.scores_fn() if self.scores_fn is not None else _t(scores).requires_grad_(True)
        B, L = s.shape
        c = clicks_BL(labels_LB)
        live = live_mask(docids_LB if h["mask_padding"] else None, n_docs, B, L)
        el = torch.where(live, element_loss(s, self.theta, c, h["tower_combination"]), torch.zeros_like(s))
        data_loss = el.sum() / B
        l2 = sum((p * p).sum() for p in self.params) * (0.5 * h["l2_loss"]) if h["l2_loss"] > 0 else 0.0
        loss = data_loss + l2
        if self.scores_fn is not None:
            data_loss.backward()
            grad = torch.cat([p.grad.reshape(-1) for p in self.params]).numpy().copy()
        else:
            (dth,) = torch.autograd.grad(data_loss, [self.theta])
            self.theta.grad = dth
            grad = None
        theta_grad = self.theta.grad.numpy().copy()
        with torch.no_grad():
            if force_grad is not None:
                for p, g in zip(self.params, self._split(force_grad)):
                    p.grad = g.clone()
            if force_theta_grad is not None:
                self.theta.grad = _t(force_theta_grad)
            if h["l2_loss"] > 0:
                for p in self.params:
                    p.grad += h["l2_loss"] * p
        mg = h["max_gradient_norm"]
        if mg > 0:
            norm = float(torch.nn.utils.clip_grad_norm_(self.params, mg))
            pnorm = float(torch.nn.utils.clip_grad_norm_([self.theta], mg))
            coef, pcoef = min(1.0, mg / (norm + 1e-6)), min(1.0, mg / (pnorm + 1e-6))
        else:
            norm = float(torch.sqrt(sum((p.grad ** 2).sum() for p in self.params)))
            pnorm = float(self.theta.grad.norm())
            coef = pcoef = 1.0
        # what the optimizers get, and per entry the sum of the magnitudes of its terms (adam_ref.moment_excess's scale)
        g_final = torch.cat([p.grad.reshape(-1) for p in self.params]).numpy().copy()
        g_terms = np.abs(g_final)
        if h["l2_loss"] > 0 and force_grad is not None:
            g_terms = (np.abs(np.asarray(force_grad, np.float64)) + h["l2_loss"] * np.abs(self.flat())) * coef
        theta_final = self.theta.grad.numpy().copy()
        self.opt.step()
        return dict(loss=float(loss.detach()), norm=norm, coef=coef, D=float(B), pnorm=pnorm, pcoef=pcoef, scores=s.detach().numpy(), grad=grad,
                    theta_grad=theta_grad, g_final=g_final, g_terms=g_terms, theta_final=theta_final)


def dnn_twin(params, theta, hyper, feature_size, hidden, features, docids_LB, act="elu"):
    """A Twin whose ranker is the oracle's DNN (oracle.ultr_oracle.dnn_forward) in float64 on one batch."""
    from oracle import ultr_oracle as O
    x = O.gather_rows(np.asarray(features, np.float32), docids_LB).double()
    L, B = np.asarray(docids_LB).shape
    p = torch.tensor(np.asarray(params, np.float64))
    tw = Twin([p], theta, hyper)
    tw.scores_fn = lambda: O.dnn_forward(tw.params[0], feature_size, hidden, x, act).view(L, B).t()
    return tw


# ------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 129, 256)
SCALES = (1.0, 8.0, 30.0)
LABEL_KINDS = ("binary", "graded", "fractional")


def make_case(L, scale, labels, B=3, seed=0):
    """scores [B, L] and theta [L] = scale x N(0, 1) (x 8, x 30: both towers saturate, with both signs), labels [L, B]: binary clicks
    at rate 0.3, graded 0 .. 4 (2, 4 clamp to 1) or fractional {0, 0.25, 0.5, 1}; list 0 has no click and list 1 is all clicked
    (where the batch has them)."""
    rng = np.random.RandomState(1000 * L + int(10 * scale) + 7 * LABEL_KINDS.index(labels) + seed)
    s = (scale * rng.normal(size=(B, L))).astype(np.float32)
    th = (scale * rng.normal(size=L)).astype(np.float32)
    if labels == "binary":
        y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    elif labels == "graded":
        y = rng.randint(0, 5, size=(L, B)).astype(np.float32)
    else:
        y = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), size=(L, B))
    y[:, 0] = 0.0
    if B > 1:
        y[:, 1] = 1.0 if labels != "graded" else 4.0
    return s, th, y
