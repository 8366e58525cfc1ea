"""Float64 torch restatement of the cube-map lookup of include/sgr_texture.h (nvdiffrast's texture() with
boundary_mode='cube' and bilinear filtering, as the reference's sky model calls it): face choice and (u, v), the seam
table DERIVED from the face orientation, the corner rule.  Autograd through `texture_ref` gives the reference texture
gradient; `tap_weights` exposes the per-sample taps (texel index, weight) the GPU tests build their bounds from."""
import math

import torch

SU = (-1, 1, 1, 1, 1, -1)
SV = (-1, -1, 1, -1, -1, -1)


def face_uv(d):
    """d [..., 3] (float64) -> face (int64), u, v (unclamped); the contract's ties: x over y, x or y over z."""
    ax, ay, az = d[..., 0].abs(), d[..., 1].abs(), d[..., 2].abs()
    zmaj = az > torch.maximum(ax, ay)
    ymaj = ~zmaj & (ay > ax)
    c = torch.where(zmaj, d[..., 2], torch.where(ymaj, d[..., 1], d[..., 0]))
    s = torch.where(zmaj | ymaj, d[..., 0], d[..., 2])
    t = torch.where(zmaj, d[..., 1], torch.where(ymaj, d[..., 2], d[..., 1]))
    face = torch.where(zmaj, 4, torch.where(ymaj, 2, 0)) + (c < 0).long()
    su = torch.tensor(SU, dtype=d.dtype, device=d.device)[face]
    sv = torch.tensor(SV, dtype=d.dtype, device=d.device)[face]
    m = 0.5 / c.abs()
    return face, s * su * m + 0.5, t * sv * m + 0.5


def texel_dir(f, R, col, row):
    """Inverse of face_uv at |major| = 1: the direction through texel centre (col, row) of face f (may lie outside)."""
    s = (2.0 * (col + 0.5) / R - 1.0) * SU[f]
    t = (2.0 * (row + 0.5) / R - 1.0) * SV[f]
    c = -1.0 if f & 1 else 1.0
    return [(c, t, s), (s, c, t), (s, t, c)][f // 2]


def seam_table():
    """{(f, e): (g, c0, c1, r0, r1)}: a tap at position k across edge e of face f (e: 0 column -1, 1 column R, 2 row -1,
    3 row R) is texel (c0 (R-1) + c1 k, r0 (R-1) + r1 k) of face g.  Derived by carrying the tap's direction into the
    face it points at, at two resolutions, and checked at every edge position."""
    table = {}
    for f in range(6):
        for e in range(4):
            found = []
            for R in (8, 7):
                pts = []
                for k in range(R):
                    col, row = {0: (-1, k), 1: (R, k), 2: (k, -1), 3: (k, R)}[e]
                    g, u, v = face_uv(torch.tensor(texel_dir(f, R, col, row), dtype=torch.float64))
                    pts.append((int(g), math.floor(float(u) * R), math.floor(float(v) * R)))
                g = pts[0][0]
                assert g != f and all(p[0] == g for p in pts)
                coef = []
                for a in (1, 2):
                    lo = pts[0][a]
                    assert lo in (0, R - 1)
                    base = 0 if lo == 0 else 1
                    step = pts[1][a] - base * (R - 1)
                    assert all(p[a] == base * (R - 1) + step * k for k, p in enumerate(pts))
                    coef += [base, step]
                found.append((g, *coef))
            assert found[0] == found[1]
            table[(f, e)] = found[0]
    return table


_SEAM = None


def _seam_tensors(device):
    global _SEAM
    if _SEAM is None:
        _SEAM = seam_table()
    t = torch.tensor([[_SEAM[(f, e)] for e in range(4)] for f in range(6)], dtype=torch.int64, device=device)
    return t  # [6, 4, 5]


def tap_weights(uv, Bt, R):
    """uv [B, H, W, 3] -> idx [B*H*W, 4] (flat texel index into tex.reshape(-1, C), -1 = no texel), w [B*H*W, 4]
    (float64; the corner rule folded in), valid [B*H*W]."""
    B = uv.shape[0]
    d = uv.reshape(B, -1, 3).to(torch.float64)
    n = d.shape[1]
    face, u, v = face_uv(d)
    valid = torch.isfinite(u) & torch.isfinite(v)
    u = torch.where(valid, u, 0.5).clamp(0, 1)
    v = torch.where(valid, v, 0.5).clamp(0, 1)
    x, y = u * R - 0.5, v * R - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    w = torch.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    cols = torch.stack([x0, x0 + 1, x0, x0 + 1], -1)
    rows = torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    f4 = face.unsqueeze(-1).expand_as(cols)
    ox = (cols < 0) | (cols >= R)
    oy = (rows < 0) | (rows >= R)
    seam = _seam_tensors(uv.device)
    e = torch.where(ox, torch.where(cols < 0, 0, 1), torch.where(rows < 0, 2, 3))
    k = torch.where(ox, rows, cols)
    ent = seam[f4, e]  # [B, n, 4, 5]
    one = ox ^ oy
    gf = torch.where(one, ent[..., 0], f4)
    gc = torch.where(one, ent[..., 1] * (R - 1) + ent[..., 2] * k, cols)
    gr = torch.where(one, ent[..., 3] * (R - 1) + ent[..., 4] * k, rows)
    missing = ox & oy
    share = (w * missing).sum(-1, keepdim=True) / 3.0
    w = torch.where(missing, 0.0, w + share)
    bt = torch.zeros(B, dtype=torch.int64, device=uv.device) if Bt == 1 else torch.arange(B, device=uv.device)
    idx = ((bt.view(B, 1, 1) * 6 + gf) * R + gr) * R + gc
    idx = torch.where(missing, -1, idx)
    w = torch.where(valid.unsqueeze(-1), w, 0.0)
    idx = torch.where(valid.unsqueeze(-1), idx, -1)
    return idx.reshape(B * n, 4), w.reshape(B * n, 4), valid.reshape(B * n)


def texture_ref(tex, uv):
    """tex [Bt, 6, R, R, C] (float64, may require grad), uv [B, H, W, 3] -> [B, H, W, C] float64."""
    Bt, _, R, _, C = tex.shape
    B, H, W, _ = uv.shape
    idx, w, _ = tap_weights(uv, Bt, R)
    flat = tex.reshape(-1, C)
    vals = flat[idx.clamp(min=0)]  # [N, 4, C]
    out = (vals * w.to(tex.dtype).unsqueeze(-1)).sum(1)
    return out.reshape(B, H, W, C)


def grad_scale(uv, dout, tex_shape):
    """S[t, c] = sum of |dL/dout| over the samples that have texel t as a footprint tap (float64): the scale of the
    gradient tolerance of t.  The float32 rounding of x = u R - 0.5 moves a tap's weight by about R * 1e-7 whatever the
    weight, so a tap of small weight is held to |dL/dout| rather than to w |dL/dout|."""
    Bt, _, R, _, C = tex_shape
    idx, w, _ = tap_weights(uv, Bt, R)
    g = dout.reshape(-1, 1, C).to(torch.float64).abs().expand(-1, 4, C)
    S = torch.zeros(Bt * 6 * R * R, C, dtype=torch.float64, device=uv.device)
    keep = idx >= 0
    S.index_add_(0, idx[keep], g[keep])
    return S.reshape(tex_shape)
