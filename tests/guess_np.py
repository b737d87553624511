"""NumPy fp64 restatement of the engine's initial-guess store (DESIGN §4.5;
mpg_engine_guess_*, solve.h): panels Z and Q = A Z with Q^T Q = I, project and
keep as specified there, the re-imaging after new matrix values. The operation
order inside a sum is NumPy's, not the kernels': the tests compare through
bounds, not bits."""
import numpy as np

U = 2.0 ** -53
MAX_DEPTH = 16


class Store:
    """matvec: x -> A x in fp64 (the matrix of the residual prologue)."""

    def __init__(self, matvec, n: int, depth: int, tol: float):
        assert 1 <= depth <= MAX_DEPTH
        self.matvec, self.n, self.depth, self.tol = matvec, n, depth, tol
        self.Z = np.zeros((n, depth), order="F")
        self.Q = np.zeros((n, depth), order="F")
        self.held = 0
        self.rho0 = self.rho1 = 0.0

    def coefficients(self, b, xbar=None):
        r = b if xbar is None else b - self.matvec(xbar)
        return r, self.Q[:, :self.held].T @ r

    def project(self, b, xbar=None):
        """x0 = xbar + Z Q^T (b - A xbar); rho0 = ||r||, rho1 the predicted ||b - A x0||"""
        r, c = self.coefficients(b, xbar)
        x0 = (np.zeros(self.n) if xbar is None else xbar) + self.Z[:, :self.held] @ c
        rr = float(r @ r)
        self.rho0, self.rho1 = np.sqrt(rr), np.sqrt(max(0.0, rr - float(c @ c)))
        return x0

    def keep(self, x) -> bool:
        """the direction of x joins the store unless it is below what the solves resolve"""
        if self.held == self.depth:
            self.held = 0  # Fischer's restart
        p = self.held
        w, d = self.matvec(x), np.array(x, dtype=np.float64)
        omega = np.linalg.norm(w)
        for _ in range(2):  # classical Gram-Schmidt, twice
            h = self.Q[:, :p].T @ w
            w = w - self.Q[:, :p] @ h
            d = d - self.Z[:, :p] @ h
        nu = np.linalg.norm(w)
        if not (np.isfinite(nu) and np.isfinite(omega)) or nu <= max(self.tol, self.n * U) * omega:
            return False
        self.Q[:, p], self.Z[:, p] = w / nu, d / nu
        self.held = p + 1
        return True

    def reimage(self, matvec) -> None:
        """new values of A: keep the held Z columns again, in order, from an empty store"""
        old = self.Z[:, :self.held].copy()
        self.matvec, self.held = matvec, 0
        for j in range(old.shape[1]):
            self.keep(old[:, j])


def orth_defect(Q) -> float:
    """max |Q^T Q - I|"""
    return float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max()) if Q.shape[1] else 0.0


def image_defects(matvec, Z, Q):
    """||Q(:, j) - A Z(:, j)|| and ||Z(:, j)|| per column"""
    return [(float(np.linalg.norm(Q[:, j] - matvec(Z[:, j]))), float(np.linalg.norm(Z[:, j])))
            for j in range(Z.shape[1])]
