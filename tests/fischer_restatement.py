"""numpy restatement of the projected initial guess (-ksp_guess_type fischer; PETSc KSPGuessFischer,
model 1). PETSc itself is not available: this class IS the specification the library is held to
(DESIGN.md "parity unpinned").

State: curl stored pairs (xtilde[i], btilde[i] = A xtilde[i]), the btilde orthonormal in the
2-norm. form(b) projects: guess = sum_i (b . btilde[i]) xtilde[i], the minimiser of ||b - A g|| over
the span. update(x), after a solve started from that guess, adds the direction x - guess
(orthonormalised in its A-image against the stored ones) unless it is zero or not finite; a full
space restarts from x alone.

`apply` is the operator: oracle.stencil, oracle.lapl or oracle.assembled with their grid bound.
"""
import numpy as np


class Fischer:
    def __init__(self, apply, maxl=10):
        self.apply, self.maxl = apply, int(maxl)
        self.xtilde, self.btilde = [], []
        self.guess = None

    @property
    def curl(self):
        return len(self.xtilde)

    def reset(self):
        self.xtilde, self.btilde = [], []

    def form(self, b):
        """The guess for b (zero while nothing is stored); kept for the next update."""
        x = np.zeros_like(b)
        for xt, bt in zip(self.xtilde, self.btilde):
            x = x + float(np.dot(b, bt)) * xt
        self.guess = x.copy()
        return x

    def update(self, x):
        """After a solve from the last formed guess. Returns curl."""
        if self.curl == self.maxl:  # space full: restart from this solution alone
            self.reset()
            bt = self.apply(x)
            norm = float(np.sqrt(np.dot(bt, bt)))
            if np.isfinite(norm) and norm != 0.0:
                self.btilde.append(bt * (1.0 / norm))
                self.xtilde.append(x * (1.0 / norm))
            return self.curl
        xt = x.copy() if self.curl == 0 else x - self.guess
        bt = self.apply(xt)
        alpha = [-float(np.dot(bt, bi)) for bi in self.btilde]
        for a, bi, xi in zip(alpha, self.btilde, self.xtilde):
            bt = bt + a * bi
            xt = xt + a * xi
        norm = float(np.sqrt(np.dot(bt, bt)))
        if np.isfinite(norm) and norm != 0.0:
            self.btilde.append(bt * (1.0 / norm))
            self.xtilde.append(xt * (1.0 / norm))
        return self.curl
