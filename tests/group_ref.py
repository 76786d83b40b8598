"""Float64 restatement of the group Cholesky (aircraft_amd/csrc/ac_group.hpp: grp_chol_column), the matrices it is measured on
and the recorded worst float32 error E32_WORST.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import numpy as np

from tests import rts_ref as R

# Worst e32 (host float32 build against float64 on identical float32-rounded matrices) over cases(), measured on the CPU:
#   L    max |dL_ij| / sqrt(M_ii)    (|L_ij| <= sqrt(M_ii): invariant under a diagonal scaling of M)
#   w    max |d(1 / L_jj)| L_jj      (relative: what the callers' triangular solves multiply by)
E32_WORST = {"L": 1.5e-7, "w": 3.1e-7}  # measured 1.47e-7, 3.06e-7

N_CASES = 8


def cases():
    """[M]: float64 arrays holding float32 values, symmetric.  Eight links of the poly chain (rts_ref.chain_records), from the
    first to the last and over the instances: M = P-_k, the matrix the smoother and the EM statistics factor, so the conditioning
    is that of the RTS grids by construction."""
    rec = R.chain_records("poly")
    T_, n = rec["X"].shape[0], rec["X"].shape[2]
    return [rec["Ppred"][1 + q * (T_ - 2) // (N_CASES - 1)][:, :, 3 * q % n].copy() for q in range(N_CASES)]


def errors(M, L32, w32):
    L = np.linalg.cholesky(M)
    return {"L": float((np.abs(L32 - L) / np.sqrt(np.diag(M))[:, None]).max()), "w": float(np.abs(w32 * np.diag(L) - 1.0).max())}
