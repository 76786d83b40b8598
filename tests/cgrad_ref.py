"""Float64 references of the coefficient gradients, shared by tests/test_host_cgrad.py and
tests/test_gpu_cgrad.py.

Central differences of  sum(lam * F)  (step) or  sum_k G_k . X_k  (rollout) through the float64 oracle built with perturbed
`coef` / `intercept` / `W`.  The base point is the FLOAT32 ROUNDING of the model data — what the handle runs.  Step
h = h_rel max(|theta_i|, 0.05) with h_rel = 1e-5; every reference comes with the one at h_rel = 3e-5, and a case first asserts
that the two agree to 1e-6 per tensor (max|a - b| / max|b|): a condition on the float64 oracle alone.
Error per tensor: max|g - g_ref| / max|g_ref|; bar 2e-5, the project's bar for the weight gradient and the composed VJP."""
import numpy as np

from tests.helpers import f32_exact, synthetic_units

BAR = 2e-5
H_REL = (1e-5, 3e-5)
H_AGREE = 1e-6
TENSORS = {"poly": ("coef", "intercept"), "linear": ("W",)}


def theta_of(ac):
    """{name: float64 array} of the model's parameters at their float32 rounding"""
    m = ac.coefficient_model
    return {k: f32_exact(getattr(m, k)) for k in TENSORS[ac.model_kind]}


def oracle_with(ac, data):
    """the float64 oracle of `ac` with other coefficients"""
    from oracle import Oracle

    return Oracle(ac.airframe_dict(), ac.model_kind, {k: np.asarray(v, np.float64) for k, v in data.items()},
                  substeps=ac.physical_integration_substeps, normalise=ac.normalise, stall_scaling=ac.stall_scaling,
                  epsilon=ac.epsilon, gravity=ac.gravity)


def units(n, seed):
    X, U = synthetic_units(n, seed=seed, flaps=True)
    lam = f32_exact(np.random.default_rng(seed + 1).normal(size=(13, n)))
    return f32_exact(X), f32_exact(U), lam


def rollout_problem(B, H):
    X0, _ = synthetic_units(B, seed=21, flaps=True)
    U = np.stack([synthetic_units(B, seed=30 + k, flaps=True)[1] for k in range(H)])
    G = f32_exact(np.random.default_rng(4).normal(size=(H + 1, 13, B)))
    return f32_exact(X0), f32_exact(U), G


def _central(ac, f, h_rel):
    """{name: theta.shape + f(.).shape}: central differences of the array-valued f(oracle) over every parameter"""
    base = theta_of(ac)
    out = {}
    for name, a in base.items():
        rows = []
        for i in range(a.size):
            h = h_rel * max(abs(float(a.flat[i])), 0.05)
            v = []
            for sgn in (1.0, -1.0):
                pert = {k: b.copy() for k, b in base.items()}
                pert[name].flat[i] += sgn * h
                v.append(f(oracle_with(ac, pert)))
            rows.append((v[0] - v[1]) / (2 * h))
        out[name] = np.stack(rows).reshape(a.shape + rows[0].shape)
    return out


def step_reference(ac, X, U, dt, lam):
    """[{name: theta.shape + (n,)} for h_rel in H_REL]: per UNIT, lam . dF/dtheta (the difference formed per unit before the
    dot product); a gradient over the first m units is the sum of the first m columns"""
    return [_central(ac, lambda o: (lam * o.state_update(X, U, dt)).sum(axis=0), h) for h in H_REL]


def rollout_reference(ac, X0, U, dt, G):
    """[{name: theta.shape + (B,)} for h_rel in H_REL]: per instance, d(sum_k G_k . X_k)/dtheta"""
    return [_central(ac, lambda o: (G * o.rollout(X0, U, dt)).sum(axis=(0, 1)), h) for h in H_REL]


def summed(ref, m=None):
    """the gradient over the first m units (all: m = None) of a per-unit reference"""
    return {k: v[..., :m].sum(axis=-1) for k, v in ref.items()}


def tensor_errors(got, want):
    return {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in want}


def check_reference(refs):
    """the condition on the reference: h_rel = 1e-5 and 3e-5 agree to 1e-6 per tensor.  -> the reference at 1e-5"""
    agree = tensor_errors(refs[0], refs[1])
    assert max(agree.values()) <= H_AGREE, ("the float64 reference does not reproduce itself", agree)
    return refs[0], agree


def split_theta(kind, flat):
    """flat (210,) or (36,) in ABI order -> {name: array}"""
    flat = np.asarray(flat, np.float64)
    if kind == "poly":
        return {"coef": flat[:204].reshape(6, 34), "intercept": flat[204:]}
    return {"W": flat.reshape(6, 6)}
