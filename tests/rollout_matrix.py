"""The rollout-engine matrix: one row per template instance that ac_rollout_f32 / ac_rollout_policy_f32 can pick for an MLP
surrogate (aircraft_amd/csrc/abi_core.hip and abi_ilqr.hip), plus the analytic models and the quadrotor for the closed loop.

The host picks by the FOLDED net:  wt = 2, 4 or 8 register tiles for a largest hidden width <= 32, <= 64 or <= 128;
nh = folded layers - 2 hidden x hidden layers.  With the matrix cores on, 1 <= nh <= 3 takes the register-resident engine
(k_nn_rollout_reg<wt, nh>), everything else the cooperative one (k_nn_rollout_coop<wt>), whose weight ring only runs when the
LDS rule streams (width 128 with four or more hidden x hidden layers).  With them off, widths <= 64 take the tiled vector-ALU
engine and width 128 the sequential k_nn_rollout<8, false>, which has no closed-loop counterpart.

tests/test_mlp_model_host.py pins (wt, folded layers, n_streamed) of every row on the CPU, so that a later change of the
fold or of the LDS rule cannot silently move a row of tests/test_gpu_rollout_engines.py to another instance."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple


@dataclass(frozen=True)
class Row:
    id: str
    hidden: Optional[Tuple[int, ...]]   # None: the shipped checkpoint (5-16-32-6, activation-free first layer)
    act: Optional[Sequence[int]]        # None: tanh on every hidden layer, identity on the output layer
    use_mfma: bool
    open_kernel: str
    policy_kernel: Optional[str]        # None: ac_rollout_policy_f32 refuses the net
    wt: int
    layers: int                         # after the fold
    n_streamed: int                     # layers the LDS plan streams (the cooperative engine runs its weight ring on them)
    H: int = 6


def _reg(id, hidden, wt, layers, act=None, n_streamed=0):
    return Row(id, hidden, act, True, "k_nn_rollout_reg", "k_nn_rollout_policy_reg", wt, layers, n_streamed)


def _coop(id, hidden, wt, layers, n_streamed=0, act=None, H=6):
    return Row(id, hidden, act, True, "k_nn_rollout_coop", "k_nn_rollout_policy_coop", wt, layers, n_streamed, H)


def _tiled8(id, hidden, wt, layers):
    return Row(id, hidden, None, False, "k_nn_rollout_tiled8", "k_nn_rollout_policy_tiled8", wt, layers, 0)


MLP_ROWS = [
    _reg("reg2x1", (32, 32), 2, 3),
    _reg("reg2x2-ragged", (24, 20, 32), 2, 4),
    _reg("reg2x3", (32,) * 4, 2, 5),
    _reg("reg4x1-ragged", (40, 64), 4, 3),
    _reg("reg4x2-ragged", (48, 24, 40), 4, 4),
    _reg("reg4x3", (64,) * 4, 4, 5),
    _reg("reg8x1-ragged", (100, 128), 8, 3),
    _reg("reg8x2-ragged", (100, 128, 72), 8, 4),
    # (the LDS plan of this net streams its three hidden blocks; the register engine keeps its weights in registers and
    # never reads that plan)
    _reg("reg8x3", (128,) * 4, 8, 5, n_streamed=3),
    _reg("reg4x2-tanh-out", (48, 24, 40), 4, 4, act=[1, 1, 1, 1]),
    _coop("coop2-16", (16,), 2, 2),
    _coop("coop2-shipped", None, 2, 2),
    _coop("coop4-1x64", (64,), 4, 2),
    _coop("coop4-5x64", (64,) * 5, 4, 6),
    # (the float64 reference of this net moves by 1.3e-5 under a one-ulp perturbation at H = 6 and by 8.8e-6 at H = 4)
    _coop("coop8-1x128", (128,), 8, 2, H=4),
    _coop("coop8-5x128-ring4", (128,) * 5, 8, 6, n_streamed=4),
    _coop("coop8-6x128-ring5", (128,) * 6, 8, 7, n_streamed=5),
    _coop("coop2-all-linear", (48, 24, 40), 2, 1, act=[0, 0, 0, 0]),
    _tiled8("tiled8-32-ragged", (24, 20, 32), 2, 4),
    _tiled8("tiled8-64-ragged", (48, 24, 40), 4, 4),
    Row("seq8-valu", (128, 128), None, False, "k_nn_rollout", None, 8, 3, 0),
]
MLP_ROW_IDS = [r.id for r in MLP_ROWS]

# closed loop only (the open loop of these is covered by tests/test_gpu_parity.py and tests/test_gpu_quadrotor.py)
ANALYTIC_ROWS = ["default", "linear", "poly", "quad"]


def mlp_data(row: Row):
    """The row's net as the product and the oracle take it (an `MlpData`)."""
    from aircraft_amd import MlpData
    from tests.helpers import golden

    if row.hidden is None:
        w = golden("scaledmodel_weights.npz")
        return MlpData([w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0], w["input_mean"], w["input_std"],
                       w["output_mean"], w["output_std"])
    base = MlpData.synthetic(row.hidden, seed=42)
    if row.act is None:
        return base
    return MlpData(base.weights, base.biases, row.act, base.input_mean, base.input_std, base.output_mean, base.output_std)
