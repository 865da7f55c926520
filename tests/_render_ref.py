"""NumPy fp32 restatement of the rendering rule ("Rendering"): what `mpe_render` draws, written the
slow and obvious way -- the support function over all 30 normals, every entity blended in draw order.  Each entity is
evaluated on its bounding box only (radius + 3 half-pixels: the outline band reaches (a + h) / cos(pi / 30)), which keeps
simple_spread N = 64 at seconds; outside it the entity covers nothing.

Every expression is an fp32 operation in the order the kernel evaluates it (the library is built with -ffp-contract=off),
so the frames agree byte for byte.  `knife` marks pixels whose sigma lies within 1e-6 of a coverage threshold (0 or 1/S).
"""
import numpy as np

F = np.float32
RES = 30
_PHI = 2 * np.pi * (np.arange(RES) + 0.5) / RES          # fp64
NX, NY = np.cos(_PHI).astype(F), np.sin(_PHI).astype(F)  # ... rounded to fp32
COS_PI_30 = np.cos(np.pi / RES)                           # fp64
KNIFE = 1e-6


def apothem(size):
    """a = size cos(pi / 30) in fp64 (size as the fp32 the descriptor holds), rounded to fp32."""
    return F(np.float64(F(size)) * COS_PI_30)


def q(v):
    """The 8-bit value a channel of intensity v gets over a white pixel at alpha 1: floor(v 255 + 1/2)."""
    return int(np.floor(F(v) * F(255) + F(0.5)))


def blend(fb, src_a, one_minus_a):
    """f' = src a + (fb / 255)(1 - a) in fp32; fb' = clamp(floor(f' 255 + 1/2), 0, 255).  fb: uint8 array [..., 3]."""
    f = src_a + (fb.astype(F) / F(255)) * one_minus_a
    return np.clip(np.floor(f * F(255) + F(0.5)), 0, 255).astype(np.uint8)


def pixel_centres(S, cx, cy):
    """x[c], y[r] of the pixel centres of a view centred on (cx, cy): row 0 is the top."""
    s = F(2) / F(S)
    idx = np.arange(S).astype(F)
    x = (F(cx) - F(1)) + (idx + F(0.5)) * s
    y = (F(cy) + F(1)) - (idx + F(0.5)) * s
    return x, y


def render_frame(pos, sizes, rgba, S, centre=(0.0, 0.0)):
    """One view: pos [E, 2], sizes [E], rgba [E, 4] (r, g, b unclamped, alpha) -> (uint8 [S, S, 3], knife bool [S, S])."""
    pos = np.asarray(pos, F)
    rgba = np.asarray(rgba, F)
    S = int(S)
    cx, cy = F(centre[0]), F(centre[1])
    h = F(1) / F(S)
    xs, ys = pixel_centres(S, cx, cy)
    fb = np.full((S, S, 3), 255, np.uint8)
    knife = np.zeros((S, S), bool)
    for e in range(pos.shape[0]):
        ex, ey = pos[e, 0], pos[e, 1]
        a = apothem(sizes[e])
        reach = float(sizes[e]) + 3.0 * float(h)
        cols = np.nonzero(np.abs(xs.astype(np.float64) - float(ex)) <= reach)[0]
        rows = np.nonzero(np.abs(ys.astype(np.float64) - float(ey)) <= reach)[0]
        if cols.size == 0 or rows.size == 0:
            continue
        r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
        dx = (xs[c0:c1] - ex)[None, :]
        dy = (ys[r0:r1] - ey)[:, None]
        dots = NX[:, None, None] * dx[None] + NY[:, None, None] * dy[None]    # [30, rows, cols]
        sigma = dots.max(axis=0) - a
        rgb = np.clip(rgba[e, :3], F(0), F(1))
        al = rgba[e, 3]
        ol = F(0.5) * al
        fill = sigma <= 0
        line = np.abs(sigma) <= h
        knife[r0:r1, c0:c1] |= (np.abs(sigma) <= KNIFE) | (np.abs(np.abs(sigma) - h) <= KNIFE)
        sub = fb[r0:r1, c0:c1]
        sub[fill] = blend(sub[fill], rgb * al, F(1) - al)
        sub[line] = blend(sub[line], (F(0.5) * rgb) * ol, F(1) - ol)
    return fb, knife


def render_frames(pos, sizes, rgba, S, cameras=(-1,)):
    """Every frame of an `mpe_render` call.  pos [K, E, 2] (the K selected worlds), rgba [K, E, 4] or [E, 4],
    cameras: per viewer the entity it centres on, -1 = the origin -> (uint8 [V, K, S, S, 3], knife bool [V, K, S, S])."""
    pos = np.asarray(pos, F)
    rgba = np.asarray(rgba, F)
    K = pos.shape[0]
    out = np.zeros((len(cameras), K, S, S, 3), np.uint8)
    knife = np.zeros((len(cameras), K, S, S), bool)
    for v, cam in enumerate(cameras):
        for k in range(K):
            centre = (0.0, 0.0) if cam < 0 else (pos[k, cam, 0], pos[k, cam, 1])
            out[v, k], knife[v, k] = render_frame(pos[k], sizes, rgba[k] if rgba.ndim == 3 else rgba, S, centre)
    return out, knife


def env_colours(env):
    """rgba [B, E, 4] of an env's entities as the rule reads them (colour channels 0-2 per world, alpha 0.5 for 'agent' names)."""
    import torch
    w = env.world
    B = env.batch_size
    out = np.zeros((B, len(w.entities), 4), F)
    for e, ent in enumerate(w.entities):
        c = ent.color
        c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        c = np.broadcast_to(np.asarray(c, F)[..., :3], (B, 3))
        out[:, e, :3] = c
        out[:, e, 3] = 0.5 if 'agent' in ent.name else 1.0
    return out


def env_sizes(env):
    return np.array([ent.size for ent in env.world.entities], F)
