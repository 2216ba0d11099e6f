"""Shared test helpers: oracle solutions for synthetic batches (CPU, float64), the symbols
include/mpcqp.h declares, the prototypes of a header, and the full (non-diagonal) weights the
parity and the interior-point edge tests share."""
import os
import re

import numpy as np

from oracle import formulation as F
from oracle import qp as QP

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcqp.h")


def _declared():
    """The name of every function include/mpcqp.h declares."""
    src = open(HEADER).read()
    return set(re.findall(r"^\s*(?:[a-zA-Z_][\w\s\*]*?)\b(mpcqp_\w+)\s*\(", src, re.M))


def _prototypes(header):
    """{name: (return type, [parameter types])} of the header at that path, comments removed; a
    type is the declaration's text less the parameter's name, "T*" for every pointer."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \*]*?)\s*\b(mpcqp_\w+)\s*\(([^)]*)\)\s*;", src, re.M):
        kinds = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm == "void" and "," not in params:
                continue
            kinds.append("T*" if "*" in prm else re.sub(r"\s*\w+$", "", prm))
        out[name] = ("T*" if "*" in ret else ret.strip(), kinds)
    return out


def _int_prototypes(header):
    """{name: [parameter types]} of a companion header, every function of which returns int."""
    protos = _prototypes(header)
    assert all(ret == "int" for ret, _ in protos.values()), protos
    return {name: kinds for name, (_, kinds) in protos.items()}


def oracle_solution(batch, b, horizon, Q=F.Q_DIAG, R=F.R_DIAG):
    """Reference-faithful formulation + exact QP optimum for robot b of a batch
    (``Q`` / ``R``: diagonals or full matrices, mpc.py:50,52)."""
    x0 = batch["x0"][b]
    xref = batch["xref"][b].reshape(-1)
    contact = batch["contact"][b].reshape(-1)
    feet = batch["feet"][b].astype(np.float64)
    rec = batch["robot"][b]
    inertia = np.array([[rec[1], rec[2], rec[3]], [rec[2], rec[4], rec[5]],
                        [rec[3], rec[5], rec[6]]], dtype=np.float32)
    normal = rec[9:12].astype(np.float64)
    o = F.formulate(x0, xref, contact, feet, inertia, float(rec[0]), horizon,
                    mu=float(rec[7]), fz_max=float(rec[8]), normal=normal, Q=Q, R=R)
    x, y, info = QP.solve_qp_dual_active_set(o["H"], o["g"], o["C"], o["lb"], o["ub"])
    return x, o, info


def rel_err_u0(u0, u0_ref):
    """Norm-wise relative error ||u0 - u0*||_inf / max(||u0*||_inf, 1e-3)."""
    return float(np.abs(np.asarray(u0, np.float64) - u0_ref).max() / max(np.abs(u0_ref).max(), 1e-3))


def _full_weights(seed, cross_leg_r=False):
    """A symmetric positive-semidefinite Q coupling the state components (the reference's
    diagonal scaled by a correlation matrix, |rho| <= 0.4: the weighting keeps the
    reference's scale, so the float32 condensing of mpc.py:213-230 perturbs the optimum
    as little as with the diagonal) and a leg-block R (or one with cross-leg terms)."""
    from mpcqp.params import Q_DIAG, R_DIAG
    rng = np.random.default_rng(seed)
    C = np.eye(13)
    for _ in range(12):
        i, j = rng.choice(12, size=2, replace=False)   # state 12 (gravity) keeps weight 0
        C[i, j] = C[j, i] = rng.uniform(-0.4, 0.4)
    w, V = np.linalg.eigh(C)
    C = V @ np.diag(np.maximum(w, 0.05)) @ V.T           # positive definite
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    sq = np.sqrt(np.asarray(Q_DIAG, np.float64))
    Q = np.outer(sq, sq) * C
    R = np.diag(R_DIAG).copy()
    for leg in range(4):
        S = rng.uniform(-0.3, 0.3, size=(3, 3))
        R[3 * leg:3 * leg + 3, 3 * leg:3 * leg + 3] += 1e-5 * (S @ S.T)
    if cross_leg_r:
        R[1, 7] = R[7, 1] = 3e-6
    return 0.5 * (Q + Q.T), 0.5 * (R + R.T)


def _cross_leg_weights(seed):
    """The full Q of _full_weights and an R coupling every pair of legs: the reference's
    diagonal scaled by a dense random correlation matrix (SPD, every cross-leg block non-zero)."""
    from mpcqp.params import R_DIAG
    Q, _ = _full_weights(seed)
    rng = np.random.default_rng(seed + 1)
    A = rng.standard_normal((12, 12))
    C = A @ A.T / 12.0 + 0.5 * np.eye(12)
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    sq = np.sqrt(np.asarray(R_DIAG, np.float64))
    R = np.outer(sq, sq) * C
    return Q, 0.5 * (R + R.T)
