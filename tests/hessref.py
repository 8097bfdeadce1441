"""NumPy restatement of the second derivatives of the PD value network of controller/vhjb.py:17-60 (TEST INFRASTRUCTURE, like netref.py):
d2V/dx2 and dy/de for relu, tanh and sin in closed form, in float64 -- or, with dtype=np.float32, the same statements evaluated in float32
on the CPU (the "CPU float build" yardstick of the parity tests: the same formulas in the same precision as the kernel, from the same inputs).

    e = wrap(x - xf); z = (e - mean)/std; a1 = z W1; h1 = act(a1); a2 = h1 W2; h2 = act(a2); y = h2 W3; V = |y|^2 + eps |e|^2
    A1 = da1/dz = W1,  A2 = da2/dz = (A1 . act'(a1)) W2,  J = dy/dz = (A2 . act'(a2)) W3
    r2 = 2y W3',  r1 = (r2 . act'(a2)) W2'                                   (the reverse sweep of the gradient)
    H_z = 2 J J' + A2 diag(r2 . act''(a2)) A2' + A1 diag(r1 . act''(a1)) A1'
    H_x = H_z / (std std') + 2 eps I,      dy/de = J / std                   (the wrap is data: d wrap = I)
"""
import numpy as np

from netref import NetRef

_ACT = {"relu": (lambda a: np.maximum(a, 0), lambda a: (a > 0).astype(a.dtype), lambda a: np.zeros_like(a)),
        "tanh": (np.tanh, lambda a: 1 - np.tanh(a) ** 2, lambda a: -2 * np.tanh(a) * (1 - np.tanh(a) ** 2)),
        "sin": (np.sin, np.cos, lambda a: -np.sin(a))}


class HessRef:
    def __init__(self, W, mean, std, xf, eps_scalar, wrap, activation):
        """W: the three weight matrices (in, out); wrap(e, dtype) -> wrapped error coordinates in that dtype."""
        self.W = [np.asarray(w, np.float64) for w in W]
        self.mean, self.std, self.xf = (np.asarray(v, np.float64).reshape(1, -1) for v in (mean, std, xf))
        self.eps, self.wrap, self.activation = float(eps_scalar), wrap, activation
        self.net = NetRef(self.W, mean, std, xf, eps_scalar, lambda e: wrap(e, np.float64))   # ReLU: forward, grad, kink margin, term scales

    def _cast(self, dtype):
        return [w.astype(dtype) for w in self.W], self.mean.astype(dtype), self.std.astype(dtype), self.xf.astype(dtype), dtype(self.eps)

    def forward(self, x, dtype=np.float64):
        (W1, W2, W3), mean, std, xf, _ = self._cast(dtype)
        act = _ACT[self.activation][0]
        e = np.asarray(self.wrap(np.asarray(x, dtype) - xf, dtype), dtype)
        z = (e - mean) / std
        a1 = z @ W1
        a2 = act(a1) @ W2
        y = act(a2) @ W3
        return dict(e=e, z=z, a1=a1, a2=a2, y=y)

    def grad(self, x, dtype=np.float64):
        """dV/dx (B, n): the reverse sweep."""
        (W1, W2, W3), mean, std, xf, eps = self._cast(dtype)
        dact = _ACT[self.activation][1]
        fw = self.forward(x, dtype)
        d2 = ((2 * fw["y"]) @ W3.T) * dact(fw["a2"])
        d1 = (d2 @ W2.T) * dact(fw["a1"])
        return (d1 @ W1.T) / std + 2 * eps * fw["e"]

    def value(self, x, dtype=np.float64):
        fw = self.forward(x, dtype)
        return (fw["y"] ** 2).sum(1) + dtype(self.eps) * (fw["e"] ** 2).sum(1)

    def hessian(self, x, dtype=np.float64):
        """-> (H (B, n, n) = d2V/dx2, dy/de (B, n, h3))"""
        (W1, W2, W3), mean, std, xf, eps = self._cast(dtype)
        _, dact, d2act = _ACT[self.activation]
        fw = self.forward(x, dtype)
        a1, a2, y = fw["a1"], fw["a2"], fw["y"]
        s1, s2 = dact(a1), dact(a2)
        A1 = W1[None, :, :]                                       # (1, n, h1)
        A2 = (A1 * s1[:, None, :]) @ W2                           # (B, n, h2)
        J = (A2 * s2[:, None, :]) @ W3                            # (B, n, h3)
        Hz = 2 * (J @ J.transpose(0, 2, 1))
        if self.activation != "relu":
            r2 = (2 * y) @ W3.T
            r1 = (r2 * s2) @ W2.T
            Hz = Hz + (A2 * (r2 * d2act(a2))[:, None, :]) @ A2.transpose(0, 2, 1) + (A1 * (r1 * d2act(a1))[:, None, :]) @ A1.transpose(0, 2, 1)
        n = std.shape[1]
        H = Hz / (std.reshape(1, n, 1) * std.reshape(1, 1, n)) + 2 * eps * np.eye(n, dtype=dtype)[None]
        assert H.dtype == dtype and J.dtype == dtype
        return H, J / std.reshape(1, n, 1)

    def kink_margin(self, x):
        """ReLU: min over the 256 hidden units of |pre-activation| / sum |terms| (NetRef.kink_margin); H and dy/de jump where it is zero."""
        return self.net.kink_margin(self.net.forward(x))
