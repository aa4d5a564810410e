"""Dense layers on encrypted rows: a public int8 matrix (Context.lwe_linear; include/ieache.h section 3n) followed by a table
lookup (Context.pbs), the partner of netlists.py and automata.py for computations on small encrypted integers.  A Dense holds

    W           int8 [n_out][n_in], the public weights
    bias        Torus32 words [n_out] added to the b term of each sum, or None
    test_poly   Torus32 [N], the activation: a row of phase t comes out as v[round(2N t)] on the first half of the circle and
                -v[. - N] on the second (the convention of ieache_pbs)
    inputs      the clear phases an input row may carry, as fractions of the torus (Fraction, or anything Fraction takes)
    slots       (spacing, offset): the decision boundaries of the activation lie at offset + k spacing

torus(x) gives the Torus32 word of a fraction x.  run() evaluates on the card through the device forms, the rows never leaving it
between the two steps; run_reference() composes tools.lwe_linear_reference with a bootstrap the caller passes; run_clear() does
the same on plain phases; margin() is the noise margin of DESIGN.md section 7 extended to weights.

Worked examples: sign_layer (the constant test polynomial: +-mu by the sign of the sum) and bivariate (x p + y through one table
of p^2 entries)."""
from fractions import Fraction

import numpy as np

from . import tools
from .evaluator import linear_weights


def torus(x):
    """the Torus32 word (a Python int in [-2^31, 2^31)) nearest to the fraction x of the torus"""
    w = int(round(Fraction(x) * (1 << 32))) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w


def _fraction(word):
    return Fraction(int(word) & 0xFFFFFFFF, 1 << 32)


class Dense:
    def __init__(self, W, bias, test_poly, inputs=None, slots=(Fraction(1, 2), Fraction(0))):
        self.W, self.bias = linear_weights(W, bias)
        self.test_poly = np.ascontiguousarray(test_poly, dtype=np.int32).reshape(-1)
        self.inputs = None if inputs is None else [Fraction(v) for v in inputs]
        self.slots = (Fraction(slots[0]), Fraction(slots[1]))

    @property
    def n_out(self):
        return self.W.shape[0]

    @property
    def n_in(self):
        return self.W.shape[1]

    # ---- on the card ----
    def run(self, ctx, x, stats=None):
        """x: host rows [batch][n_in][n+1] -> host rows [batch][n_out][n+1]; or a torch int32 tensor on the context's device,
        [batch][n_in][lwe_stride] -> a tensor [batch][n_out][lwe_stride], so that layers chain without a copy.  lwe_linear_device
        then pbs_device on the context's stream; the sums stay on the device.  stats: that of the bootstrap."""
        import torch
        p, stride = ctx.params, ctx.lwe_stride
        on_device = isinstance(x, torch.Tensor)
        if on_device:
            dx = x.contiguous()
            assert dx.dtype == torch.int32 and dx.shape[-2:] == (self.n_in, stride)
            dx = dx.reshape(-1, self.n_in, stride)
        else:
            rows = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, self.n_in, p.n + 1)
            padded = np.zeros(rows.shape[:2] + (stride,), dtype=np.int32)
            padded[..., :p.n + 1] = rows
            dx = torch.from_numpy(padded).cuda()
        batch = dx.shape[0]
        dev = dx.device
        dw = torch.from_numpy(self.W).to(dev)
        dbias = None if self.bias is None else torch.from_numpy(self.bias).to(dev)
        dtv = torch.from_numpy(self.test_poly).to(dev)
        dmid = torch.empty((batch, self.n_out, stride), dtype=torch.int32, device=dev)
        dout = torch.empty((batch, self.n_out, stride), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the context's stream is not ordered after the copies above
        if batch:
            ctx.lwe_linear_device("lwe", batch, self.n_out, self.n_in, dw.data_ptr(), None if dbias is None else dbias.data_ptr(), dx.data_ptr(),
                                  dmid.data_ptr())
            ctx.pbs_device(batch * self.n_out, dmid.data_ptr(), dtv.data_ptr(), 1, None, dout.data_ptr(), stats=stats)
        return dout if on_device else dout.cpu().numpy()[..., :p.n + 1]

    # ---- the same composed from references ----
    def run_reference(self, params, x, pbs):
        """tools.lwe_linear_reference, then pbs(rows [count][n+1], test_poly [N]) -> rows [count][n+1] (the caller's reference of
        the bootstrap, e.g. the oracle's stages) -> [batch][n_out][n+1]"""
        sums = tools.lwe_linear_reference(params, x, self.W, self.bias, "lwe")
        out = np.asarray(pbs(sums.reshape(-1, params.n + 1), self.test_poly), dtype=np.int32)
        return out.reshape(sums.shape[0], self.n_out, params.n + 1)

    # ---- on plain numbers ----
    def clear_phases(self, values):
        """values [batch][n_in] (or [n_in]) clear input phases as fractions of the torus -> [batch][n_out] lists of Fractions
        in [0, 1): sum_j W[i][j] v_j + bias[i] mod 1"""
        vals = [[Fraction(v) for v in row] for row in np.asarray(values, dtype=object).reshape(-1, self.n_in)]
        out = []
        for row in vals:
            out.append([(sum(int(w) * v for w, v in zip(self.W[i], row)) + (_fraction(self.bias[i]) if self.bias is not None else 0)) % 1
                        for i in range(self.n_out)])
        return out

    def activation(self, phase):
        """the Torus32 word the bootstrap's output encrypts for a clear input phase (a fraction of the torus)"""
        N = self.test_poly.shape[0]
        idx = int(round(Fraction(phase) * 2 * N)) % (2 * N)
        return int(self.test_poly[idx]) if idx < N else -int(self.test_poly[idx - N])

    def run_clear(self, values):
        """values [batch][n_in] clear phases -> int64 [batch][n_out]: the words the outputs encrypt, noise aside"""
        return np.array([[self.activation(t) for t in row] for row in self.clear_phases(values)], dtype=np.int64).reshape(-1, self.n_out)

    # ---- noise ----
    def reachable_phases(self, i):
        """the clear phases neuron i can see when every input carries one of self.inputs"""
        assert self.inputs is not None, "Dense: the margin needs the inputs' alphabet"
        sums = {_fraction(self.bias[i]) if self.bias is not None else Fraction(0)}
        for w in self.W[i]:
            sums = {(s + int(w) * v) % 1 for s in sums for v in self.inputs}
        return sorted(sums)

    def gap(self, i):
        """the smallest distance of a reachable clear phase of neuron i to a slot boundary"""
        spacing, offset = self.slots
        d = [(t - offset) % spacing for t in self.reachable_phases(i)]
        return min(min(x, spacing - x) for x in d)

    def neuron_margins(self, V, sigma_delta, rounding):
        """per neuron (gap - |sum_j w_j| 4 sigma_delta) / sqrt(||w||^2 V + rounding): V the variance of an input row's noise,
        sigma_delta the standard deviation of the per-key offset all rows share -- it adds coherently, so it enters with the SUM of
        the weights, taken at 4 of its deviations against the neuron -- and rounding the variance of the mod switch
        """
        W = self.W.astype(np.int64)
        return [(float(self.gap(i)) - abs(int(W[i].sum())) * 4.0 * sigma_delta) / float(np.sqrt(float((W[i] ** 2).sum()) * V + rounding))
                for i in range(self.n_out)]

    def margin(self, V, sigma_delta, rounding):
        """the smallest neuron's margin in standard deviations"""
        return min(self.neuron_margins(V, sigma_delta, rounding))


def sign_layer(W, bias, inputs=None, mu=1 << 29, N=1024):
    """Neurons with the sign activation: the constant test polynomial, +mu for a sum on the first half of the circle and -mu on
    the second (the gate bootstrap's table); boundaries at 0 and 1/2.  bias: Torus32 words (torus(x) of a fraction)."""
    return Dense(W, bias, np.full(N, int(mu), dtype=np.int64).astype(np.int32), inputs=inputs, slots=(Fraction(1, 2), Fraction(0)))


def bivariate(f, p, params, scale=None):
    """A function of two encrypted numbers x, y < p through ONE lookup: the sum x p + y, then the table of p^2 entries
    f(x, y) (Torus32 words, or with `scale` integers that are multiplied by it).  Inputs are encoded as tools.lut_test_poly
    encodes a message of a p^2-entry table, m at phase m / (2 p^2); 2 p^2 must divide N.  One neuron, weights (p, 1)."""
    p = int(p)
    table = [int(f(x, y)) * (1 if scale is None else int(scale)) for x in range(p) for y in range(p)]
    words = np.array([torus(Fraction(t, 1 << 32)) for t in table], dtype=np.int64).astype(np.int32)
    step = Fraction(1, 2 * p * p)
    return Dense([[p, 1]], None, tools.lut_test_poly(params, words), inputs=[m * step for m in range(p)], slots=(step, step / 2))
