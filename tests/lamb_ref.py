"""float64 restatement of one LAMB step with global gradient-norm clipping over a list of tensors (vipant_amd/module/lamb.py,
vipant_amd/csrc/lamb.hip), and the relative bound of the fp32 gradient norm, derived from the kernels' accumulation and not from
their results.

G: a thread of the chunk's workgroup adds its 32 squares (chunk 8192, 256 threads) to one fp32 accumulator with one fma each -- 32
roundings in sequence; the workgroup's tree adds 6 levels inside a wave and 2 across the four waves -- 8 more.  All terms are
non-negative, so a chunk's partial sum is within (32 + 8) u of its value, relatively, u = 2^-24.  The partials are folded in fp64
(at most nchunks roundings of 2^-53: nothing at this scale), the square root (fp64 as well) halves the relative error, and the
conversion to fp32 adds one rounding:  |G - G_64| <= (40 / 2 + 1) u G = G_REL G.  The clip factor c = min(1, max_grad_norm / (G + 1e-6))
is evaluated in fp32 from that G: max_grad_norm's rounding, the sum, the quotient -- three more: C_REL = G_REL + 3 u."""
import numpy as np

U = 2.0 ** -24
G_REL = 21 * U
C_REL = G_REL + 3 * U


def lamb_step_f64(tensors, *, beta1, beta2, max_grad_norm):
    """`tensors`: dicts with p, g, m, v (arrays), lr, wd, eps, adapt and step (the count AFTER this step).  -> (G, c, [(p1, m1, v1)])
    in float64.  wd and adapt are the per-tensor values, after `exclude_bias_and_norm` has been applied."""
    G = np.sqrt(sum(float(np.sum(np.asarray(t["g"], dtype=np.float64) ** 2)) for t in tensors))
    c = min(1.0, max_grad_norm / (G + 1e-6)) if max_grad_norm > 0 else 1.0
    out = []
    for t in tensors:
        p, g, m, v = (np.asarray(t[k], dtype=np.float64) for k in "pgmv")
        g = c * g
        m1 = m + (1.0 - beta1) * (g - m)
        v1 = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** t["step"], 1.0 - beta2 ** t["step"]
        u = (m1 / bc1) / (np.sqrt(v1 / bc2) + t["eps"]) + t["wd"] * p
        pn, un = np.sqrt(np.sum(p * p)), np.sqrt(np.sum(u * u))
        phi = pn / un if (t["adapt"] and pn > 0 and un > 0) else 1.0
        out.append((p - t["lr"] * phi * u, m1, v1))
    return G, c, out
