"""Torch restatement of the arithmetic that include/sgr_actor_pose.h declares, for K records at once, in float32 (the
op-by-op parts are held bit for bit against it) or float64 (its autograd gradient is the yardstick of the HIP backward).
The small-angle branches are evaluated on safe arguments so that autograd never meets a 0/0 in a branch not taken.

``poses(records, input_trans, input_rots, opt_trans, opt_rots, ego, dtype)``: ``records`` is the numpy plan
(street_gaussians_amd.actor_pose.RECORD_DTYPE); the tensors are [F, O, .] or flat [n_cells, .]; ``opt_*`` None means
tracking is not optimised.  Returns [K, 7]."""
import numpy as np
import torch


def qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz,
                        aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw), -1)


def qconj(a):
    return a * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=a.dtype, device=a.device)


def mul_theta_cs(q, c, s):
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack((qw * c - qz * s, qx * c + qy * s, qy * c - qx * s, qz * c + qw * s), -1)


def normalize(q):
    n = torch.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
    return q / n.clamp_min(1e-12)[..., None]


def _norm3(v):
    """|v| with the zero subgradient at v = 0 (what the kernel's backward does there)."""
    sq = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def _sinc_half(h, x):
    """sin(x / 2) / x with h = x / 2, and 0.5 - x^2 / 48 below 1e-3."""
    small = x < 1e-3
    xs = torch.where(small, torch.ones_like(x), x)
    hs = torch.where(small, torch.ones_like(h), h)
    return torch.where(small, 0.5 - x * x / 48.0, torch.sin(hs) / xs)


def slerp(q0, q1, r):
    """[K, 4] x [K, 4] x [K] -> [K, 4]."""
    a, b = normalize(q0), normalize(q1)
    p = qmul(qconj(a), b)
    sg = torch.where(p[..., 0] < 0, -torch.ones_like(p[..., 0]), torch.ones_like(p[..., 0]))
    p = p * sg[..., None]
    s = _norm3(p[..., 1:])
    h = torch.atan2(s, p[..., 0])
    ang = 2.0 * h
    c1 = _sinc_half(h, ang)
    v = p[..., 1:] / c1[..., None] * r[..., None]
    m = _norm3(v)
    hm = 0.5 * m
    c2 = _sinc_half(hm, m)
    e = torch.cat([torch.cos(hm)[..., None], v * c2[..., None]], -1)
    return qmul(a, e)


def matrix_to_quaternion(R):
    """[3, 3] -> [4], the header's form of general_utils.py:159-218."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.reshape(9).unbind(0)
    d = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22])
    q_abs = torch.where(d > 0, torch.sqrt(d.clamp_min(0)), torch.zeros_like(d))
    i = int(torch.argmax(q_abs))  # the first largest
    sq = q_abs[i] * q_abs[i]
    rows = ([sq, m21 - m12, m02 - m20, m10 - m01], [m21 - m12, sq, m10 + m01, m02 + m20],
            [m02 - m20, m10 + m01, sq, m12 + m21], [m10 - m01, m20 + m02, m21 + m12, sq])
    return torch.stack(rows[i]) / (2.0 * q_abs[i].clamp_min(0.1))


def lerp(ta, tb, wa, wb, wd):
    return (ta * wa[..., None] + tb * wb[..., None]) / wd[..., None]


def world(qe, R, t, Q, T):
    out_rot = qmul(qe.expand_as(Q), Q)
    out_trans = torch.stack([R[i, 0] * T[..., 0] + R[i, 1] * T[..., 1] + R[i, 2] * T[..., 2] + t[i] for i in range(3)], -1)
    return out_rot, out_trans


def _sample(s, it, ir, ot, orr, dtype, dev, cs=None):
    idx = lambda k: torch.from_numpy(s[k].astype(np.int64)).to(dev)
    w = lambda k: torch.from_numpy(s[k].astype(np.float32)).to(dev).to(dtype)
    a, b = idx("a"), idx("b")
    ta, tb = it[a], it[b]
    if ot is not None:
        ta, tb = ta + ot[a], tb + ot[b]
    T = lerp(ta, tb, w("wa"), w("wb"), w("wd"))
    if ot is not None:
        t1, t2 = orr[idx("th1")], orr[idx("th2")]
        c1, s1, c2, s2 = cs if cs is not None else (torch.cos(t1), torch.sin(t1), torch.cos(t2), torch.sin(t2))
        qa = mul_theta_cs(ir[a], c1, s1)
        qb = mul_theta_cs(qa, c2, s2)
    else:
        qa, qb = ir[a], ir[b]
    return T, slerp(qa, qb, w("r")), qa, qb


def poses(records, input_trans, input_rots, opt_trans, opt_rots, ego, dtype=torch.float64, parts=False, cs=None):
    """``cs`` = (cos t1, sin t1, cos t2, sin t2) of sample 0 replaces the library calls (the bitwise comparison of mul_theta
    takes the kernel's own values).  ``parts`` adds a dict of the intermediates of sample 0."""
    dev = input_trans.device
    it = input_trans.reshape(-1, 3).to(dtype)
    ir = input_rots.reshape(-1, 4).to(dtype)
    ot = opt_trans.reshape(-1, 3).to(dtype) if opt_trans is not None else None
    orr = opt_rots.reshape(-1).to(dtype) if opt_rots is not None else None
    E = ego.to(dtype)
    s = records["s"]
    T, Q, qa, qb = _sample(s[:, 0], it, ir, ot, orr, dtype, dev, cs)
    T0 = T
    two = torch.from_numpy(records["n_samples"] == 2).to(dev)
    if bool(two.any()):
        s1 = s[:, 1].copy()
        one = records["n_samples"] != 2
        s1[one] = s[:, 0][one]  # a valid stand-in where there is no second sample; not selected below
        T2, Q2, _, _ = _sample(s1, it, ir, ot, orr, dtype, dev)
        w = lambda k, fill: torch.from_numpy(np.where(one, np.float32(fill), records[k]).astype(np.float32)).to(dev).to(dtype)
        To = lerp(T, T2, w("Wa", 1.0), w("Wb", 0.0), w("Wd", 1.0))
        Qo = slerp(Q, Q2, w("R", 0.0))
        T = torch.where(two[:, None], To, T)
        Q = torch.where(two[:, None], Qo, Q)
    qe = matrix_to_quaternion(E[:3, :3])
    out_rot, out_trans = world(qe, E[:3, :3], E[:3, 3], Q, T)
    out = torch.cat([out_rot, out_trans], -1)
    if parts:
        return out, dict(T=T0, qa=qa, qb=qb, qe=qe, Q=Q)
    return out
