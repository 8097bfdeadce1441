"""NumPy restatement of the soft-PD value network of the notebooks (SoftPDValueApproximator) and of its second derivative with respect to
the state (TEST INFRASTRUCTURE, like hessref.py): d2V/dx2 for tanh, sin and relu in closed form, in float64 -- or, with dtype=np.float32, the
same statements evaluated in float32 on the CPU (the "CPU float build" yardstick of the parity tests).

    e = wrap(x - xf); z = (e - mean)/std; a1 = z W1 + b1; h1 = act(a1); a2 = h1 W2 + b2; h2 = act(a2); a3 = h2 W3 + b3; V = act(a3) . w4 + b4
    d3 = w4 . act'(a3),  r2 = d3 W3',  r1 = (r2 . act'(a2)) W2',  dV/dz = (r1 . act'(a1)) W1'        (the reverse sweep of the gradient)
    A1 = da1/dz = W1,  A2 = da2/dz = (A1 . act'(a1)) W2,  A3 = da3/dz = (A2 . act'(a2)) W3
    H_z = A3 diag(w4 . act''(a3)) A3' + A2 diag(r2 . act''(a2)) A2' + A1 diag(r1 . act''(a1)) A1'
    H_x = H_z / (std std')                                                     (no eps term; the wrap is data: d wrap = I)
"""
import numpy as np

from hessref import _ACT


class SoftHessRef:
    def __init__(self, params, mean, std, xf, wrap, activation):
        """params: W1 (n,h1), b1, W2, b2, W3, b3, w4 (h3,) or (h3,1), b4 (scalar or (1,)); wrap(e, dtype) -> wrapped error coordinates."""
        W1, b1, W2, b2, W3, b3, w4, b4 = (np.asarray(p, np.float64) for p in params)
        self.p = [W1, b1.reshape(1, -1), W2, b2.reshape(1, -1), W3, b3.reshape(1, -1), w4.reshape(1, -1), b4.reshape(())]
        self.mean, self.std, self.xf = (np.asarray(v, np.float64).reshape(1, -1) for v in (mean, std, xf))
        self.wrap, self.activation = wrap, activation

    def _cast(self, dtype):
        return [q.astype(dtype) for q in self.p], self.mean.astype(dtype), self.std.astype(dtype), self.xf.astype(dtype)

    def forward(self, x, dtype=np.float64):
        (W1, b1, W2, b2, W3, b3, w4, b4), mean, std, xf = self._cast(dtype)
        act = _ACT[self.activation][0]
        e = np.asarray(self.wrap(np.asarray(x, dtype) - xf, dtype), dtype)
        z = (e - mean) / std
        a1 = z @ W1 + b1
        a2 = act(a1) @ W2 + b2
        a3 = act(a2) @ W3 + b3
        V = (act(a3) * w4).sum(1) + b4
        return dict(e=e, z=z, a1=a1, a2=a2, a3=a3, V=V)

    def value(self, x, dtype=np.float64):
        return self.forward(x, dtype)["V"]

    def _reverse(self, fw, P):
        W1, b1, W2, b2, W3, b3, w4, b4 = P
        dact = _ACT[self.activation][1]
        r2 = (w4 * dact(fw["a3"])) @ W3.T
        r1 = (r2 * dact(fw["a2"])) @ W2.T
        return r2, r1

    def grad(self, x, dtype=np.float64):
        """dV/dx (B, n): the reverse sweep."""
        P, mean, std, xf = self._cast(dtype)
        fw = self.forward(x, dtype)
        _, r1 = self._reverse(fw, P)
        return ((r1 * _ACT[self.activation][1](fw["a1"])) @ P[0].T) / std

    def hessian(self, x, dtype=np.float64):
        """-> H (B, n, n) = d2V/dx2"""
        P, mean, std, xf = self._cast(dtype)
        W1, b1, W2, b2, W3, b3, w4, b4 = P
        _, dact, d2act = _ACT[self.activation]
        fw = self.forward(x, dtype)
        a1, a2, a3 = fw["a1"], fw["a2"], fw["a3"]
        s1, s2 = dact(a1), dact(a2)
        r2, r1 = self._reverse(fw, P)
        A1 = W1[None, :, :]                                       # (1, n, h1)
        A2 = (A1 * s1[:, None, :]) @ W2                           # (B, n, h2)
        A3 = (A2 * s2[:, None, :]) @ W3                           # (B, n, h3)
        T = lambda A: A.transpose(0, 2, 1)                        # noqa: E731
        Hz = (A3 * (w4 * d2act(a3))[:, None, :]) @ T(A3) + (A2 * (r2 * d2act(a2))[:, None, :]) @ T(A2) + (A1 * (r1 * d2act(a1))[:, None, :]) @ T(A1)
        n = std.shape[1]
        H = Hz / (std.reshape(1, n, 1) * std.reshape(1, 1, n))
        assert H.dtype == dtype
        return H
