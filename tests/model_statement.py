"""The float64 statement of GaussianModel's reset family (scene/gaussian_model.py:532-722) and of the three steps the training loops
build from it: what materialrefgs_amd/model.py and csrc/mrgs_model_reset.hip are tested against, itself tested against the reference's
own methods (tests/golden/reference_model.npz).  numpy only.

A model is a dict of float64 arrays -- opacity, refl_strength, roughness [P,1], f_dc [P,1,3], f_rest [P,15,3], ori_color [P,3], scaling
[P,2] -- plus the three settings refl_msk_thr, rough_msk_thr, enlarge_scale.  Every method returns (new model, margin): the groups it
replaces are new arrays, the others are shared; `margin` is the smallest relative distance |q - t| / t of any decision quantity q (a
sigmoid that is compared with a threshold t) from its threshold, over all rows -- inputs with margin >= 1e-3 decide the same way in fp32
and in float64.  Thresholds and the constants a, b enter as their fp32 images, as they do in the reference (a Python scalar meets an fp32
tensor) and in the kernel.

`literal=True` writes logit(sigmoid(v)) on the unchanged side of CAP and FLOOR, as the reference's min / max formulation does
(reset_opacity0, reset_refl, reset_refl_strength2); the kernel keeps v there bit for bit.  (The reference's reset_opacity1 copies the raw
row itself, so LIFT's unchanged side is v either way.)

Tolerances (eps = 2^-23, one unit in the last place of an fp32 library function; a basic operation rounds to eps / 2):
  logit_tol   an fp32 evaluation of x = log(s / (1 - s)) with s = sigmoid(v) = 1 / (1 + exp(-v)): exp within eps, the sum and the quotient
              eps / 2 each, so |ds| / s <= eps (1 - s) + eps <= 2 eps.  1 - s inherits ds: relative ds / (1 - s) + eps / 2.  The log's
              argument s / (1 - s) is off by ds / (s (1 - s)) + eps relative, <= 2 eps / (1 - s) + eps, which the log turns into the same
              ABSOLUTE error, plus eps |x| for the log itself: |dx| <= eps (1 + |x| + 2 / (s (1 - s))) (using 1 / (1 - s) <= 1 / (s (1 - s))).
              The same bound covers a constant L(a) evaluated in fp32 from the fp32 image of a (s = a, ds / s = eps / 2).
  jitter_tol  v + ((u a) 2 - a): the product and the difference are below 0.4 in size and round to eps / 2 of that, the last sum to
              eps / 2 |x|: 4 2^-24 max(1, |x|) holds with room.
  enlarge_tol log(exp(v) a): exp within eps, the product eps / 2, the log turns the 1.5 eps into an absolute error and adds eps |x|:
              eps (2 + |x|).
  jitter_const_tol  c = a + (u - 0.5) b carries |dc| <= 2^-24 (|a| + |b|) (the difference is exact or rounds at 2^-25, the product rounds
              at 2^-24 |b| / 2, the sum at 2^-24 c); 1 - c inherits it; the quotient and the log as in logit_tol:
              2^-24 (|a| + |b|) / (c (1 - c)) + eps (1 + |x|).
"""
import math

import numpy as np

CAP, FLOOR, LIFT, CONST, FILL, JITTER, JITTER_CONST, ENLARGE = range(8)
KEEP_EXCLUSIVE, KEEP_REFL_ABOVE, KEEP_REFL_BELOW, KEEP_ROUGH_ABOVE = 1, 2, 4, 8
EPS = 2.0 ** -23
GROUPS = {"opacity": (1,), "refl_strength": (1,), "roughness": (1,), "f_dc": (1, 3), "f_rest": (15, 3), "ori_color": (3,), "scaling": (2,)}
SETTINGS = {"refl_msk_thr": 0.02, "rough_msk_thr": 0.1, "enlarge_scale": 1.5}


def f32(x):
    """The fp32 image of a Python scalar, as a Python float."""
    return float(np.float32(x))


def L(a):
    return math.log(a / (1.0 - a))


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def logit(s):
    return np.log(s / (1.0 - s))


def _distance(q, t):
    q = np.asarray(q, dtype=np.float64)
    return float(np.min(np.abs(q - t) / abs(t))) if q.size else math.inf


def keep_rows(keep, refl_raw, rough_raw, exclusive, refl_thr, rough_thr):
    """(bool [P]: rows for which any selected condition holds, margin)."""
    P = np.asarray(refl_raw).reshape(-1).shape[0]
    rows, margin = np.zeros(P, dtype=bool), math.inf
    if keep & KEEP_EXCLUSIVE and exclusive is not None:
        rows |= np.asarray(exclusive).reshape(-1).astype(bool)
    if keep & (KEEP_REFL_ABOVE | KEEP_REFL_BELOW):
        s, t = sigmoid(refl_raw).reshape(-1), f32(refl_thr)
        margin = min(margin, _distance(s, t))
        if keep & KEEP_REFL_ABOVE:
            rows |= s > t
        if keep & KEEP_REFL_BELOW:
            rows |= s < t
    if keep & KEEP_ROUGH_ABOVE:
        s, t = sigmoid(rough_raw).reshape(-1), f32(rough_thr)
        margin = min(margin, _distance(s, t))
        rows |= s > t
    return rows, margin


def apply_rule(rule, v, a=0.0, b=0.0, u=None, literal=False):
    """(new values float64 of v's shape, bool mask of the elements the rule left as they were, margin)."""
    v = np.asarray(v, dtype=np.float64)
    same, margin = np.zeros(v.shape, dtype=bool), math.inf
    af, bf = f32(a), f32(b)
    if rule in (CAP, FLOOR, LIFT):
        s = sigmoid(v)
        margin = _distance(s, af)
        change = {CAP: s > af, FLOOR: s < af, LIFT: ~(s > af)}[rule]
        same = ~change
        untouched = logit(s) if (literal and rule != LIFT) else v
        return np.where(change, L(a), untouched), same, margin
    if rule == CONST:
        return np.full(v.shape, L(a)), same, margin
    if rule == FILL:
        return np.full(v.shape, af), same, margin
    if rule == JITTER:
        return v + ((np.asarray(u, dtype=np.float64) * af) * 2.0 - af), same, margin
    if rule == JITTER_CONST:
        c = np.clip(af + (np.asarray(u, dtype=np.float64) - 0.5) * bf, 0.0, 1.0)
        with np.errstate(divide="ignore"):
            return logit(c), same, margin
    if rule == ENLARGE:
        return np.log(np.exp(v) * af), same, margin
    raise ValueError(f"unknown rule {rule}")


def reset_item(src, rule, keep, a, b, u, refl_raw, rough_raw, exclusive, refl_thr, rough_thr, literal=False):
    """One item of mrgs_model_reset: (new [P,...] float64, bool [P,...] of the elements that must equal src bit for bit, margin)."""
    src = np.asarray(src, dtype=np.float64)
    rows, m0 = keep_rows(keep, refl_raw, rough_raw, exclusive, refl_thr, rough_thr)
    new, same, m1 = apply_rule(rule, src, a, b, u, literal)
    shape = (-1,) + (1,) * (src.ndim - 1)
    r = np.broadcast_to(rows.reshape(shape), src.shape)
    return np.where(r, src, new), same | r, min(m0, m1)


# ---- tolerances (see the module docstring) ---------------------------------------------------------------------------------------
def logit_tol(x):
    x = np.asarray(x, dtype=np.float64)
    s = sigmoid(x)
    return EPS * (1.0 + np.abs(x) + 2.0 / (s * (1.0 - s)))


def jitter_tol(x):
    return 4.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(x))


def enlarge_tol(x):
    return EPS * (2.0 + np.abs(x))


def jitter_const_tol(x, a, b):
    c = sigmoid(x)
    return 2.0 ** -24 * (abs(a) + abs(b)) / (c * (1.0 - c)) + EPS * (1.0 + np.abs(x))


# ---- the methods -----------------------------------------------------------------------------------------------------------------
def _item(model, group, rule, keep, a=0.0, b=0.0, u=None, exclusive=None, literal=False):
    new, _same, margin = reset_item(model[group], rule, keep if exclusive is not None else keep & ~KEEP_EXCLUSIVE, a, b, u, model["refl_strength"],
                                    model["roughness"], exclusive, model["refl_msk_thr"], model["rough_msk_thr"], literal)
    return dict(model, **{group: new}), margin


def reset_opacity0(model, literal=False):
    return _item(model, "opacity", CAP, 0, 0.01, literal=literal)


def reset_opacity1(model, exclusive=None):
    return _item(model, "opacity", LIFT, KEEP_EXCLUSIVE, 0.9, exclusive=exclusive)


def reset_refl(model, exclusive=None, rst_value=None, literal=False):
    return _item(model, "refl_strength", FLOOR, KEEP_EXCLUSIVE, 0.1 if rst_value is None else rst_value, exclusive=exclusive, literal=literal)


def reset_refl_strength(model, reset_value=0.01):
    return _item(model, "refl_strength", CONST, 0, reset_value)


def reset_refl_strength2(model, reset_value=0.1, literal=False):
    return _item(model, "refl_strength", FLOOR, 0, reset_value, literal=literal)


def reset_roughness(model, reset_value=0.1):
    return _item(model, "roughness", CONST, 0, reset_value)


def reset_ori_color(model, u, reset_value=0.5, noise_level=0.05):
    return _item(model, "ori_color", JITTER_CONST, 0, reset_value, noise_level, u=u)


def reset_features(model, reset_value_dc=0.0, reset_value_rest=0.0):
    model, _ = _item(model, "f_dc", FILL, 0, reset_value_dc)
    return _item(model, "f_rest", FILL, 0, reset_value_rest)


def dist_color(model, u, exclusive=None):
    return _item(model, "f_dc", JITTER, KEEP_EXCLUSIVE | KEEP_REFL_ABOVE, 0.4, u=u, exclusive=exclusive)


def dist_albedo(model, u, exclusive=None):
    return _item(model, "ori_color", JITTER, KEEP_EXCLUSIVE | KEEP_REFL_ABOVE, 0.4, u=u, exclusive=exclusive)


def reset_scale(model, exclusive=None):
    return _item(model, "scaling", ENLARGE, KEEP_EXCLUSIVE | KEEP_REFL_BELOW | KEEP_ROUGH_ABOVE, model["enlarge_scale"], exclusive=exclusive)


def enlarge_refl_scales(model, ret_raw=True, exclusive=None):
    new, margin = reset_scale(model, exclusive)
    return (new["scaling"] if ret_raw else np.exp(new["scaling"])), margin


def _chain(model, steps):
    margin = math.inf
    for step in steps:
        model, m = step(model)
        margin = min(margin, m)
    return model, margin


def normal_propagation_step(model, u=None, exclusive=None, with_dist_color=True):
    steps = [lambda m: reset_opacity1(m, exclusive)] + ([lambda m: dist_color(m, u, exclusive)] if with_dist_color else []) + \
            [lambda m: reset_scale(m, exclusive)]
    return _chain(model, steps)


def opacity_reset_step(model, exclusive=None, rst_value=None, literal=False):
    return _chain(model, [lambda m: reset_opacity0(m, literal), lambda m: reset_refl(m, exclusive, rst_value, literal)])


def material_reset_step(model, u, init_roughness_value, features=False):
    steps = [lambda m: reset_ori_color(m, u), lambda m: reset_refl_strength(m, 0.1), lambda m: reset_roughness(m, init_roughness_value)]
    return _chain(model, steps + ([reset_features] if features else []))


def random_model(P, seed, lo=-6.0, hi=6.0, min_margin=1e-3, exclusive_fraction=0.25):
    """A model of fp32-exact raw values in [lo, hi], an exclusive mask and uniforms, resampled until every method below decides with
    margin >= min_margin.  Returns (model, exclusive bool [P], {group: u of the group's shape})."""
    rng = np.random.default_rng(seed)
    while True:
        model = {g: rng.uniform(lo, hi, (P,) + s).astype(np.float32).astype(np.float64) for g, s in GROUPS.items()}
        model.update(SETTINGS)
        exclusive = rng.random(P) < exclusive_fraction
        u = {g: rng.random((P,) + GROUPS[g]).astype(np.float32).astype(np.float64) for g in ("f_dc", "ori_color")}
        margins = [reset_opacity0(model)[1], reset_opacity1(model, exclusive)[1], reset_refl(model, exclusive)[1], reset_refl(model, exclusive, 0.1)[1],
                   reset_refl_strength2(model)[1], dist_color(model, u["f_dc"], exclusive)[1], reset_scale(model, exclusive)[1]]
        if min(margins) >= min_margin:
            return model, exclusive, u
