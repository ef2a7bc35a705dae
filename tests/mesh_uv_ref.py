"""The oracle of the UV atlas ops (include/mvd.h: mvd_op_mesh_vertex_normals / _texel_bake / _texture_dilate / _render_uv), numpy
only, written from the definitions in that header: chart edge functions in Python / int64 integers, everything else in float64.
The texel -> face map is tests/mesh_ref.raster on the chart coordinates; the visibility test reuses mesh_ref's integers with the
rule "the winning face IS the texel's face"."""
import numpy as np

from tests import mesh_ref as R

SUB, ONE, KMAX = R.SUB, R.ONE, R.KMAX


def uv_to_atlas(uv, Ht, Wt):
    uv = np.asarray(uv, dtype=np.float64)
    return np.stack([np.rint(16.0 * (uv[:, 0] * Wt - 0.5)), np.rint(16.0 * ((1.0 - uv[:, 1]) * Ht - 0.5))], -1).astype(np.int32)


def tex_face(uv_xy, face_uv, Ht, Wt):
    """[Ht,Wt] int32: the rasteriser on the chart coordinates with key 1 everywhere (ties: the smallest face index)."""
    uv_xy = np.asarray(uv_xy)
    fid, _, bad = R.raster(uv_xy[None], np.ones((1, len(uv_xy)), np.int32), np.asarray(face_uv), Ht, Wt)
    assert bad == 0
    return fid[0]


def _edges(x, y, px, py):
    """(e[3], A, swapped) of one triangle at integer points px, py (arrays), after the orientation swap; e[k] of swapped vertex k."""
    x, y = [int(a) for a in x], [int(a) for a in y]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    swapped = A < 0
    if swapped:
        x[1], x[2], y[1], y[2], A = x[2], x[1], y[2], y[1], -A
    e = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = np.int64(x[b] - x[a]), np.int64(y[b] - y[a])
        e.append(dx * (py - y[a]) - dy * (px - x[a]))
    return e, A, swapped


def texel_barycentrics(uv_xy, face_uv, tf):
    """b [Ht,Wt,3] float64 (NaN without a face): b[..., k] = e_k / A of corner k of the face AS STORED, exact integer ratios
    rounded once to float64."""
    uv_xy, face_uv = np.asarray(uv_xy).astype(np.int64), np.asarray(face_uv)
    Ht, Wt = tf.shape
    b = np.full((Ht, Wt, 3), np.nan)
    for f in np.unique(tf[tf >= 0]):
        ii, jj = np.nonzero(tf == f)
        t = face_uv[f]
        e, A, swapped = _edges(uv_xy[t, 0], uv_xy[t, 1], jj.astype(np.int64) * ONE, ii.astype(np.int64) * ONE)
        order = [0, 2, 1] if swapped else [0, 1, 2]  # e[k] of the swapped triangle belongs to stored corner order[k]
        for k in range(3):
            b[ii, jj, order[k]] = e[k].astype(np.float64) / float(A)
    return b


def texel_points(b, tf, faces, attr):
    """sum_k b_k attr[faces[f][k]] per texel, float64 [Ht,Wt,C] (NaN without a face)."""
    faces, attr = np.asarray(faces), np.asarray(attr, dtype=np.float64)
    f = np.clip(tf, 0, None)
    out = (b[..., None] * attr[faces[f]]).sum(2)
    out[tf < 0] = np.nan
    return out


def bake(img01, txy, tkey, face_id, pix_key, tf, pos, nrm, centres, power=2.0, bias=4096, two_sided=False, fill=(0.5, 0.5, 0.5)):
    """The fusion per texel given the per-view integers txy [N,Ht,Wt,2] / tkey [N,Ht,Wt] and the float64 surface points and
    normals: dict of texture [Ht,Wt,3], weight_sum, spread, n_seen [Ht,Wt], visible, w [N,Ht,Wt]; img01 [N,H,W,3]."""
    txy, tkey, face_id, pix_key = (np.asarray(a).astype(np.int64) for a in (txy, tkey, face_id, pix_key))
    pos, nrm, centres = (np.asarray(a, dtype=np.float64) for a in (pos, nrm, centres))
    N, Ht, Wt = tkey.shape
    _, H, W, _ = img01.shape
    chart = tf >= 0
    vis, w, col = np.zeros((N, Ht, Wt), bool), np.zeros((N, Ht, Wt)), np.zeros((N, Ht, Wt, 3))
    p, nr = np.where(chart[..., None], pos, 0.0), np.where(chart[..., None], nrm, 0.0)
    for n in range(N):
        xs, ys, kv = txy[n, ..., 0], txy[n, ..., 1], tkey[n]
        pj, pi = (xs + ONE // 2) >> SUB, (ys + ONE // 2) >> SUB
        inside = chart & R.vertex_ok(xs, ys, kv) & (pj >= 0) & (pj < W) & (pi >= 0) & (pi < H)
        pjc, pic = np.clip(pj, 0, W - 1), np.clip(pi, 0, H - 1)
        fid, pk = face_id[n, pic, pjc], pix_key[n, pic, pjc]
        vis[n] = inside & (fid >= 0) & ((fid == tf) | (kv + bias >= pk))
        d = centres[n] - p
        nn, dd = (nr * nr).sum(-1), (d * d).sum(-1)
        good = (nn > 0) & (dd > 0)
        cs = np.where(good, (nr * d).sum(-1) / np.sqrt(np.where(good, nn * dd, 1.0)), 0.0)
        cs = np.minimum(np.abs(cs) if two_sided else np.maximum(cs, 0.0), 1.0)
        w[n] = np.where(cs > 0, cs ** power, 0.0)
        j0, i0 = xs >> SUB, ys >> SUB
        fx, fy = ((xs & (ONE - 1)) / ONE)[..., None], ((ys & (ONE - 1)) / ONE)[..., None]
        ja, jb, ia, ib = np.clip(j0, 0, W - 1), np.clip(j0 + 1, 0, W - 1), np.clip(i0, 0, H - 1), np.clip(i0 + 1, 0, H - 1)
        top = img01[n, ia, ja] * (1 - fx) + img01[n, ia, jb] * fx
        bot = img01[n, ib, ja] * (1 - fx) + img01[n, ib, jb] * fx
        col[n] = top * (1 - fy) + bot * fy
    w = w * vis
    sw = w.sum(0)
    seen = sw > 0
    texture = np.where(seen[..., None], (w[..., None] * col).sum(0) / np.where(seen, sw, 1.0)[..., None], np.asarray(fill, dtype=np.float64))
    var = (w * ((col - texture[None]) ** 2).mean(-1)).sum(0)
    spread = np.where(seen, np.sqrt(var / np.where(seen, sw, 1.0)), np.nan)
    return {"texture": texture, "weight_sum": sw, "spread": spread, "n_seen": vis.sum(0), "visible": vis, "w": w}


NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))  # N, NE, E, SE, S, SW, W, NW; row 0 is the top


def dilate(texture, valid, passes):
    """(texture float64 [Ht,Wt,3], valid bool [Ht,Wt]) after ``passes`` rounds."""
    tex, val = np.asarray(texture, dtype=np.float64).copy(), np.asarray(valid).astype(bool).copy()
    Ht, Wt = val.shape
    for _ in range(passes):
        s, c = np.zeros_like(tex), np.zeros((Ht, Wt), np.int64)
        pt, pv = np.pad(tex, ((1, 1), (1, 1), (0, 0))), np.pad(val, 1)
        for di, dj in NEIGHBOURS:
            nv = pv[1 + di:1 + di + Ht, 1 + dj:1 + dj + Wt]
            s += np.where(nv[..., None], pt[1 + di:1 + di + Ht, 1 + dj:1 + dj + Wt], 0.0)
            c += nv
        grow = ~val & (c > 0)
        tex = np.where(grow[..., None], s / np.maximum(c, 1)[..., None], tex)
        val = val | grow
    return tex, val


def normal_sums(verts, faces):
    """(S [Nv,3]: the sum of cross(v1 - v0, v2 - v0) over the incident faces; P [Nv,3]: the same sum of |a_y b_z| + |a_z b_y| ...,
    the magnitudes that enter each component; deg [Nv]) in float64."""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    fn = np.cross(a, b)
    fp = np.abs(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) + np.abs(a[:, [2, 0, 1]] * b[:, [1, 2, 0]])
    S, P, deg = np.zeros_like(v), np.zeros_like(v), np.zeros(len(v), np.int64)
    for c in range(3):
        np.add.at(S, f[:, c], fn)
        np.add.at(P, f[:, c], fp)
        np.add.at(deg, f[:, c], 1)
    return S, P, deg


def vertex_normals(verts, faces):
    S, _, _ = normal_sums(verts, faces)
    length = np.linalg.norm(S, axis=1, keepdims=True)
    return np.where(length > 0, S / np.where(length > 0, length, 1.0), 0.0)


def render_barycentrics(xy, key, face_id, faces, perspective=True, depth=None):
    """b [N,H,W,3] float64 of the covered pixels (NaN elsewhere), corner k of the winning face as stored.  perspective: g_k / sum g
    with g_k = e_k key_k in Python integers; else the affine e_k / A.  depth [N,Nv]: weights e_k / Z_k instead of the keys (the
    textbook form, for the oracle's self-check)."""
    xy, key, face_id, faces = np.asarray(xy).astype(np.int64), np.asarray(key).astype(np.int64), np.asarray(face_id), np.asarray(faces)
    N, H, W = face_id.shape
    b = np.full((N, H, W, 3), np.nan)
    for n in range(N):
        for f in np.unique(face_id[n][face_id[n] >= 0]):
            ii, jj = np.nonzero(face_id[n] == f)
            ids = faces[f]
            e, A, swapped = _edges(xy[n, ids, 0], xy[n, ids, 1], jj.astype(np.int64) * ONE, ii.astype(np.int64) * ONE)
            order = [0, 2, 1] if swapped else [0, 1, 2]
            if perspective and depth is None:  # Python integers: products up to 2^59, a correctly rounded quotient
                g = [[int(v) * int(key[n, ids[order[k]]]) for v in e[k]] for k in range(3)]
                for k in range(3):
                    b[n, ii, jj, order[k]] = [a / (p + q + r) for a, p, q, r in zip(g[k], g[0], g[1], g[2])]
                continue
            g = [e[k].astype(np.float64) / (depth[n, ids[order[k]]] if perspective else 1.0) for k in range(3)]
            for k in range(3):
                b[n, ii, jj, order[k]] = g[k] / (g[0] + g[1] + g[2])
    return b


def sample_texture(texture, u, v):
    """Bilinear, clamp to edge, of texture [Ht,Wt,3] at (u Wt - 0.5, (1 - v) Ht - 0.5); returns (colour, tx, ty)."""
    tex = np.asarray(texture, dtype=np.float64)
    Ht, Wt = tex.shape[:2]
    tx, ty = u * Wt - 0.5, (1.0 - v) * Ht - 0.5
    x0, y0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - x0)[..., None], (ty - y0)[..., None]
    ja, jb = np.clip(x0, 0, Wt - 1).astype(int), np.clip(x0 + 1, 0, Wt - 1).astype(int)
    ia, ib = np.clip(y0, 0, Ht - 1).astype(int), np.clip(y0 + 1, 0, Ht - 1).astype(int)
    top = tex[ia, ja] * (1 - fx) + tex[ia, jb] * fx
    bot = tex[ib, ja] * (1 - fx) + tex[ib, jb] * fx
    return top * (1 - fy) + bot * fy, tx, ty


def render(xy, key, face_id, faces, face_uv, uv, texture, background=(1.0, 1.0, 1.0), perspective=True):
    """images [N,H,W,3] float64 in [-1, 1] and the texel coordinates (tx, ty) [N,H,W] (NaN where uncovered)."""
    face_id, face_uv, uv = np.asarray(face_id), np.asarray(face_uv), np.asarray(uv, dtype=np.float64)
    b = render_barycentrics(xy, key, face_id, faces, perspective)
    mask = face_id >= 0
    bz = np.where(mask[..., None], b, 0.0)
    uvc = uv[face_uv[np.clip(face_id, 0, None)]]  # [N,H,W,3,2]
    u, v = (bz * uvc[..., 0]).sum(-1), (bz * uvc[..., 1]).sum(-1)
    col, tx, ty = sample_texture(texture, u, v)
    col = np.where(mask[..., None], col, np.asarray(background, dtype=np.float64))
    return 2.0 * col - 1.0, np.where(mask, tx, np.nan), np.where(mask, ty, np.nan)


_SCENE = {}


def uv_scene():
    """The scene of the per-op tests, computed once and shared (treat it as read-only): icosphere(1, 0.3) with an icosphere(0, 0.1)
    in front of it (100 faces) and one far vertex that no camera sees, under ring_cameras(4, 48, 56); the oracle's projection,
    raster, normals and camera centres; triangle_atlas charts at 64 x 48 and 40 x 40 (Wt x Ht) with their texel -> face maps."""
    if not _SCENE:
        from morphablediffusion_amd import mesh as MS
        H, W = 48, 56
        K, RT = R.ring_cameras(4, H, W)
        v0, f0 = R.icosphere(1, 0.3)
        v1, f1 = R.icosphere(0, 0.1, (0.08, -0.05, 0.43))
        verts = np.concatenate([v0, v1, [[0.0, 5.0, 0.0]]]).astype(np.float32)
        faces = np.concatenate([f0, f1 + len(v0)]).astype(np.int32)
        P = R.project(verts, K, RT, 2.0)
        face_id, pix_key, bad = R.raster(P["xy"], P["key"], faces, H, W)
        assert bad == 0
        atlases = {}
        for Ht, Wt in ((48, 64), (40, 40)):
            uv, face_uv = MS.triangle_atlas(len(faces), Ht, Wt)
            uv_xy = uv_to_atlas(uv, Ht, Wt)
            atlases[(Ht, Wt)] = dict(uv=uv, face_uv=face_uv, uv_xy=uv_xy, tex_face=tex_face(uv_xy, face_uv, Ht, Wt))
        _SCENE.update(H=H, W=W, N=len(K), K=K, RT=RT, verts=verts, faces=faces, z_near=2.0, xy=P["xy"], key=P["key"], proj=P,
                      face_id=face_id, pix_key=pix_key, normals=vertex_normals(verts, faces), centres=R.camera_centres(RT),
                      n_big=len(f0), atlases=atlases)
    return _SCENE
