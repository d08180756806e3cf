"""The fused AllReduce + residual add + RMSNorm in numpy over 16-bit patterns: fp32 adds, fp64 y."""
import numpy as np

DTYPES = ("fp16", "bf16")
MANT = {"fp16": 10, "bf16": 7}
EMIN = {"fp16": -14, "bf16": -126}
EPS = np.float32(1e-5)


def decode(bits, dt):
    if dt == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def encode(a32, dt):
    """fp32 -> the element type, rounded to nearest even."""
    if dt == "fp16":
        return a32.astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def inputs(seed, n, rows, cols, dt, residual):
    """x of every rank and the residual: magnitudes in [2^-3, 2^2], random signs; gamma in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    val = lambda: encode(np.exp2(rng.uniform(-3, 2, (rows, cols))).astype(np.float32) *
                         rng.choice(np.float32([-1, 1]), (rows, cols)), dt)
    xs = [val() for _ in range(n)]
    res = val() if residual else None
    gamma = encode(rng.uniform(0.5, 2.0, cols).astype(np.float32), dt)
    return xs, res, gamma


def model(xs, res, gamma, dt):  # -> (res_out patterns, y in fp64)
    s = decode(xs[0], dt)
    for x in xs[1:]:
        s = s + decode(x, dt)  # one fp32 add each, rank order
    if res is not None:
        s = s + decode(res, dt)
    zq = encode(s, dt)
    z = decode(zq, dt).astype(np.float64)
    ms = (z * z).sum(axis=1, keepdims=True) / z.shape[1]
    return zq, z / np.sqrt(ms + np.float64(EPS)) * decode(gamma, dt).astype(np.float64)


def ulps(got, want64, dt):  # |got - want| in units of the element type's spacing at `want`
    e = np.floor(np.log2(np.maximum(np.abs(want64), 2.0 ** EMIN[dt])))
    return np.abs(decode(got, dt).astype(np.float64) - want64) / np.exp2(e - MANT[dt])


class Guarded:
    """A [rows][cols] device tensor of the element type between two 64-byte runs of 0xA5."""
    PAD = 64

    def __init__(self, torch, rows, cols, dt, bits=None):
        nbytes = rows * cols * 2
        self.whole = torch.full((nbytes + 2 * self.PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        tdt = torch.float16 if dt == "fp16" else torch.bfloat16
        self.t = self.whole[self.PAD:self.PAD + nbytes].view(tdt).view(rows, cols)
        if bits is not None:
            self.t.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))

    def read(self):  # (patterns, guards intact)
        raw = self.whole.cpu().numpy()
        ok = bool((raw[:self.PAD] == 0xA5).all() and (raw[-self.PAD:] == 0xA5).all())
        return raw[self.PAD:-self.PAD].view(np.uint16).reshape(self.t.shape), ok


def judge(xs, res, gamma, dt, got_y, got_res):
    """The failed checks of one rank's results (patterns; got_res None without a residual)."""
    zq, y64 = model(xs, res, gamma, dt)
    wrong, worst = 0 if got_res is None else int((got_res != zq).sum()), float(ulps(got_y, y64, dt).max())
    return (["res_out differs from the model in %d elements" % wrong] if wrong else []) + \
           ([] if worst <= 2.0 else ["y is %.3f ulp from the fp64 reference" % worst])
