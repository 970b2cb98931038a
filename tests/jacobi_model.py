"""The cyclic Jacobi eigen-solver of the solvers' models (sim3_model H6, pnp_model P5, init_model I4 / I9, newpts_model N5):
the definition csrc/jacobi.h is compared with.  Pairs row by row, one rotation per pair whose entry is not zero, and a sweep
starts only while off > JACOBI_STOP * (diag + 2 off); float64, one rounding per operation, in the order written here.

jacobi_sym is jacobi4_lane statement for statement, for any m; jacobi_sym_batch is the same arithmetic over a batch of
problems at once (the leading axis), which changes no bit (tests/test_jacobi.py).  Each caller passes its own sweep count."""
import math

import numpy as np

JACOBI_STOP = 1e-32


def jacobi_sym(A, sweeps):
    """A: symmetric m x m as a list of lists of Python floats, overwritten (the eigenvalues stay on its diagonal); returns V
    with the eigenvectors in its columns"""
    m = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(m)] for i in range(m)]
    for _ in range(sweeps):
        off = diag = 0.0
        for p in range(m):
            for q in range(p + 1, m):
                off = off + A[p][q] * A[p][q]
        for i in range(m):
            diag = diag + A[i][i] * A[i][i]
        if off <= JACOBI_STOP * (diag + 2.0 * off):
            break
        for p in range(m):
            for q in range(p + 1, m):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                app, aqq = A[p][p], A[q][q]
                theta = (aqq - app) / (2.0 * apq)
                den = abs(theta) + math.sqrt(theta * theta + 1.0)
                t = 1.0 / den if theta >= 0.0 else -1.0 / den
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for r in range(m):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        A[r][p] = A[p][r] = c * arp - s * arq
                        A[r][q] = A[q][r] = s * arp + c * arq
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - s * vrq
                    V[r][q] = s * vrp + c * vrq
                A[p][p], A[q][q] = app - t * apq, aqq + t * apq
                A[p][q] = A[q][p] = 0.0
    return V


def jacobi_sym_batch(A, sweeps):
    """jacobi_sym on symmetric [B][m][m] at once.  Returns (eigenvalues [B][m] = the diagonal, V [B][m][m] with eigenvectors
    in columns), unsorted."""
    A = np.array(A, np.float64)
    B, m = A.shape[:2]
    V = np.broadcast_to(np.eye(m), (B, m, m)).copy()
    pairs = [(p, q) for p in range(m) for q in range(p + 1, m)]
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            off = np.zeros(B)
            for p, q in pairs:
                off = off + A[:, p, q] * A[:, p, q]
            diag = np.zeros(B)
            for i in range(m):
                diag = diag + A[:, i, i] * A[:, i, i]
            active = ~(off <= JACOBI_STOP * (diag + 2.0 * off))
            if not active.any():
                break
            for p, q in pairs:
                apq, app, aqq = A[:, p, q].copy(), A[:, p, p].copy(), A[:, q, q].copy()
                do = active & ~(apq == 0.0)
                if not do.any():
                    continue
                theta = (aqq - app) / (2.0 * apq)
                den = np.abs(theta) + np.sqrt(theta * theta + 1.0)
                t = np.where(theta >= 0.0, 1.0 / den, -1.0 / den)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = A[:, :, p].copy(), A[:, :, q].copy()
                newp = c[:, None] * arp - s[:, None] * arq
                newq = s[:, None] * arp + c[:, None] * arq
                newp[:, p], newp[:, q] = app - t * apq, 0.0
                newq[:, q], newq[:, p] = aqq + t * apq, 0.0
                newp = np.where(do[:, None], newp, arp)
                newq = np.where(do[:, None], newq, arq)
                A[:, :, p] = newp
                A[:, p, :] = newp
                A[:, :, q] = newq
                A[:, q, :] = newq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(do[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(do[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.diagonal(A, axis1=1, axis2=2).copy(), V
