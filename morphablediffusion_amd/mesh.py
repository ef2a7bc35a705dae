"""A coloured mesh out of generated views (include/mvd.h: mvd_op_mesh_project / _raster / _vertex_colors, csrc/k_mesh.hip): the
conditioning mesh is rasterised into the N target cameras with exact integer visibility, and each vertex takes the weighted mean
of the view colours that see it.  Not a reference feature (its only 3-D output is a NeuS2 data folder).

  read_mesh         vertices and triangles of an OBJ / PLY file          vertex_normals   area-weighted, host, float64
  rasterize_mesh    face_id / pix_key / depth / mask of every view       texture_mesh     per-vertex colours and their statistics
  write_ply         binary little-endian, uchar colours                  overlay_views    the mesh drawn over the views (plain torch)

UV texture atlases (mvd_op_mesh_vertex_normals / _texel_bake / _texture_dilate / _render_uv, csrc/k_mesh_uv.hip):

  read_mesh_uv      an OBJ with vt: verts, faces, uv, face_uv            triangle_atlas   per-triangle charts for a mesh without UVs
  uv_to_atlas       uv -> chart coordinates in 1/16 texel (float64)      vertex_normals_device   the normals of a batch of frames
  bake_texture      the views fused per texel, then dilated              render_textured  the textured mesh in any cameras
  reprojection_metrics   the atlas rendered back, scored by image_metrics   write_obj     OBJ + MTL + PNG

Closest points and surface distances (mvd_op_mesh_closest_point, csrc/k_closest.hip):

  closest_point     per point: face, barycentrics, point, distance        surface_distance   scan-to-mesh distance and its statistics

What is exact: everything after the projection (coverage, depth order, visibility, n_seen) is integer arithmetic.  What is not
computed: UV unwrapping beyond triangle_atlas, mip-maps, seam-aware blending across charts, the input photo as a 17th view (its
camera is not in the batch).  The FLAME mesh ends at the head, so colour on hair and shoulders is not recovered."""
import struct

import numpy as np
import torch

from . import engine as E
from .generate_face import read_ply_header

KMAX = E.MESH_KMAX

_PLY_CODES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
              "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d", "float64": "d"}


def _fan(poly, tris):
    for k in range(1, len(poly) - 1):
        tris.append((poly[0], poly[k], poly[k + 1]))


def _read_obj(path):
    vs, tris = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                p = line.split()
                vs.append([float(p[1]), float(p[2]), float(p[3])])
            elif line.startswith("f "):
                poly = []
                for tok in line.split()[1:]:
                    i = int(tok.split("/")[0])  # v, v/vt, v//vn, v/vt/vn
                    poly.append(i - 1 if i > 0 else len(vs) + i)  # a negative index counts back from the vertices read so far
                if len(poly) < 3:
                    raise ValueError(f"{path}: a face with fewer than 3 vertices")
                _fan(poly, tris)
    return vs, tris


def _read_ply(path):
    with open(path, "rb") as f:
        fmt, elements = read_ply_header(f, path)
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unknown PLY format {fmt!r}")
        end = "<" if fmt == "binary_little_endian" else ">"
        vs, tris = None, []
        for name, count, props in elements:
            names = [p[0] for p in props]
            if name == "vertex":
                if any(p[1] == "list" for p in props):
                    raise ValueError(f"{path}: list property on vertices is not supported")
                if not all(a in names for a in "xyz"):
                    raise ValueError(f"{path}: vertex element has no x/y/z")
            index_prop = next((n for n in ("vertex_indices", "vertex_index") if n in names), None) if name == "face" else None
            if name == "face" and index_prop is None:
                raise ValueError(f"{path}: face element has no vertex_indices / vertex_index list")
            rows = []
            for _ in range(count):  # one record: scalars and lists in property order
                rec = {}
                if fmt == "ascii":
                    tok = f.readline().split()
                    if not tok:
                        raise ValueError(f"{path}: truncated {name} data")
                    at = 0
                    for p in props:
                        if p[1] == "list":
                            n = int(tok[at])
                            rec[p[0]] = [int(float(t)) for t in tok[at + 1:at + 1 + n]]
                            at += 1 + n
                        else:
                            rec[p[0]] = float(tok[at])
                            at += 1
                else:
                    for p in props:
                        if p[1] == "list":
                            cs = struct.Struct(end + _PLY_CODES[p[2]])
                            n = cs.unpack(_exact(f, cs.size, path, name))[0]
                            it = struct.Struct(end + _PLY_CODES[p[3]] * n)
                            rec[p[0]] = list(it.unpack(_exact(f, it.size, path, name)))
                        else:
                            s = struct.Struct(end + _PLY_CODES[p[1]])
                            rec[p[0]] = s.unpack(_exact(f, s.size, path, name))[0]
                rows.append(rec)
            if name == "vertex":
                vs = [[r["x"], r["y"], r["z"]] for r in rows]
            elif name == "face":
                for r in rows:
                    poly = [int(i) for i in r[index_prop]]
                    if len(poly) < 3:
                        raise ValueError(f"{path}: a face with fewer than 3 vertices")
                    _fan(poly, tris)
        if vs is None:
            raise ValueError(f"{path}: no vertex element")
        return vs, tris


def _exact(f, n, path, name):
    raw = f.read(n)
    if len(raw) != n:
        raise ValueError(f"{path}: truncated {name} data")
    return raw


def read_mesh(path):
    """(verts float64 [Nv,3], faces int32 [Nf,3]) of a Wavefront OBJ or a PLY file (ascii, binary little / big endian), vertices
    as stored (``generate_face.read_mesh_vertices`` returns the same array).  OBJ ``f`` lines in the v, v/vt, v//vn and v/vt/vn
    forms, negative indices; PLY ``face`` elements with a vertex_indices / vertex_index list.  Polygons are fan-triangulated."""
    path = str(path)
    if path.lower().endswith(".obj"):
        vs, tris = _read_obj(path)
    elif path.lower().endswith(".ply"):
        vs, tris = _read_ply(path)
    else:
        raise ValueError(f"{path}: expected a .ply or .obj mesh")
    if not vs:
        raise ValueError(f"{path}: no vertices")
    verts = np.asarray(vs, dtype=np.float64)
    faces = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: a face index is outside the {len(verts)} vertices")
    return verts, faces.astype(np.int32)


def vertex_normals(verts, faces):
    """Unit vertex normals [Nv,3] (float64, numpy), area-weighted: the sum of the cross products of the incident faces.  A vertex
    without a face, or with cancelling ones, gets the zero vector (which weighs 0 in texture_mesh)."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, f[:, c], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)


def _device_of(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda:0")


def _as_tensor(a, dtype):
    return a.detach().to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype)


def _cameras(K, RT):
    K, RT = _as_tensor(K, torch.float64).cpu(), _as_tensor(RT, torch.float64).cpu()
    if K.dim() != 3 or K.shape[1] < 3 or K.shape[2] < 3 or RT.dim() != 3 or tuple(RT.shape[1:]) != (3, 4) or K.shape[0] != RT.shape[0]:
        raise ValueError(f"cameras: K must be [N,3,3] (or [N,4,4]) and RT [N,3,4], got {tuple(K.shape)} and {tuple(RT.shape)}")
    return K[:, :3, :3].contiguous(), RT.contiguous()


def default_z_near(verts, RT):
    """Half the smallest camera-space depth of any vertex over the views (float64 on the host)."""
    v = _as_tensor(verts, torch.float64).cpu()
    RT = _as_tensor(RT, torch.float64).cpu()
    z = torch.einsum("nj,vj->nv", RT[:, 2, :3], v) + RT[:, 2, 3:4]
    zmin = float(z.min())
    if not zmin > 0.0:
        raise ValueError(f"a vertex lies at or behind a camera plane (smallest depth {zmin}): pass z_near")
    return 0.5 * zmin


def _mesh_args(verts, faces):
    v = _as_tensor(verts, torch.float64)
    f = _as_tensor(faces, torch.int64)
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"verts must be [Nv,3], got {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"faces must be [Nf,3], got {tuple(f.shape)}")
    return v, f.to(torch.int32)


def _raster(verts, faces, K, RT, H, W, z_near, dev):
    xy, key = E.op_mesh_project(verts, K, RT, z_near, device=dev)
    face_id, pix_key, bad = E.op_mesh_raster(xy, key, faces.to(dev), H, W, device=dev)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{nbad} of the {faces.shape[0]} faces have a vertex index outside [0, {verts.shape[0]})")
    return xy, key, face_id, pix_key


def rasterize_mesh(verts, faces, K, RT, H, W, z_near=None):
    """The mesh in the N cameras: {"face_id" [N,H,W] int32 (-1 background), "pix_key" [N,H,W] int32 (0 background), "depth"
    [N,H,W] float32 = z_near KMAX / pix_key (inf on background), "mask" [N,H,W] bool (covered), "z_near"}, device tensors.
    verts [Nv,3] in the world frame of ``batch["vertices"]``, K [N,3,3] or [N,4,4], RT [N,3,4] world -> camera; pixel (i, j) has
    its centre at (u, v) = (j, i).  ``~mask`` is a background mask for ``image_metrics``; ``mask`` a ``loss_mask``."""
    v, f = _mesh_args(verts, faces)
    K3, RT = _cameras(K, RT)
    z_near = default_z_near(v, RT) if z_near is None else float(z_near)
    dev = _device_of(verts, K, RT)
    _, _, face_id, pix_key = _raster(v, f, K3, RT, int(H), int(W), z_near, dev)
    mask = face_id >= 0
    depth = torch.where(mask, (z_near * KMAX) / pix_key.clamp(min=1).double(), torch.full((), float("inf"), device=dev, dtype=torch.float64))
    return {"face_id": face_id, "pix_key": pix_key, "depth": depth.float(), "mask": mask, "z_near": z_near}


def texture_mesh(views, verts, faces, K, RT, power=2.0, bias=4096, two_sided=False, fill=(0.5, 0.5, 0.5), z_near=None):
    """Per-vertex colours out of N views [N,3,H,W] or [N,H,W,3] (float in [-1, 1] or uint8) of the mesh under cameras K, RT:
    {"colors" [Nv,3] in [0, 1], "n_seen" [Nv] int32 (views that see the vertex), "weight_sum" [Nv], "spread" [Nv] (weighted RMS
    deviation of the view colours from the fused one; NaN where no view weighs), "visible" [N,Nv] bool, "face_id", "mask"}
    (device tensors) and the floats "consistency" (mean spread over the vertices with n_seen >= 2: the multi-view consistency of
    the views, lower is better, no ground truth needed) and "coverage" (share of the vertices with a positive weight sum).
    Weight of view n at a vertex: max(0, cos)^power (|cos|^power with two_sided) between the vertex normal and the direction to
    the camera; a vertex behind the surface by more than ``bias`` depth keys of the nearest pixel's winner is not seen."""
    if not torch.is_tensor(views):
        views = torch.as_tensor(np.asarray(views))
    if views.dim() != 4 or (views.shape[1] == 3) == (views.shape[3] == 3):
        raise ValueError(f"views must be [N,3,H,W] or [N,H,W,3], got {tuple(views.shape)}")
    N, H, W = (views.shape[0], views.shape[2], views.shape[3]) if views.shape[1] == 3 else tuple(views.shape[:3])
    v, f = _mesh_args(verts, faces)
    K3, RT = _cameras(K, RT)
    if K3.shape[0] != N:
        raise ValueError(f"{N} views but {K3.shape[0]} cameras")
    z_near = default_z_near(v, RT) if z_near is None else float(z_near)
    dev = _device_of(views, verts, K)
    xy, key, face_id, pix_key = _raster(v, f, K3, RT, H, W, z_near, dev)
    normals = torch.from_numpy(vertex_normals(v.cpu().numpy(), f.cpu().numpy()))
    centres = -torch.einsum("nji,nj->ni", RT[:, :, :3], RT[:, :, 3])  # -R^T t
    out = E.op_mesh_vertex_colors(views, xy, key, f.to(dev), face_id, pix_key, v, normals, centres, power=power, bias=bias,
                                  two_sided=two_sided, fill=fill, device=dev)
    multi = out["n_seen"] >= 2
    res = {"colors": out["color"], "n_seen": out["n_seen"], "weight_sum": out["weight_sum"], "spread": out["spread"],
           "visible": out["visible"], "face_id": face_id, "mask": face_id >= 0,
           "consistency": float(out["spread"][multi & ~torch.isnan(out["spread"])].double().mean()) if bool(multi.any()) else float("nan"),
           "coverage": float((out["weight_sum"] > 0).double().mean())}
    return res


def write_ply(path, verts, faces, colors=None):
    """A binary little-endian PLY: float x y z (double where verts are float64), uchar red green blue = rint(255 c) of colours
    in [0, 1] when given, and the triangles as ``list uchar int vertex_indices``."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype("<i4").reshape(-1, 3)
    ftype = "double" if v.dtype == np.float64 else "float"
    fields = [("x", "<f8" if ftype == "double" else "<f4"), ("y", "<f8" if ftype == "double" else "<f4"),
              ("z", "<f8" if ftype == "double" else "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property {ftype} {a}" for a in "xyz"]
    if colors is not None:
        c = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        if c.shape != (len(v), 3):
            raise ValueError(f"colors must be [{len(v)},3], got {c.shape}")
        c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(len(v), dtype=fields)
    for i, a in enumerate("xyz"):
        rec[a] = v[:, i]
    if colors is not None:
        for i, a in enumerate(("red", "green", "blue")):
            rec[a] = c8[:, i]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def overlay_views(views, mask, face_id, alpha=0.5, tint=(0.1, 0.8, 0.3)):
    """uint8 strip [H, N W, 3]: the views with the mesh silhouette tinted (``alpha``) and the triangle edges -- covered pixels whose
    right or lower neighbour belongs to another face or to none -- drawn in the tint.  views [N,3,H,W] or [N,H,W,3], float in [-1, 1] or
    uint8; mask / face_id [N,H,W] as rasterize_mesh returns them.  Plain torch on the tensors' device."""
    if views.dim() != 4 or (views.shape[1] == 3) == (views.shape[3] == 3):
        raise ValueError(f"views must be [N,3,H,W] or [N,H,W,3], got {tuple(views.shape)}")
    x = views if views.shape[3] == 3 else views.permute(0, 2, 3, 1)
    x = x.float() / 255.0 if views.dtype == torch.uint8 else (x.float().clamp(-1.0, 1.0) + 1.0) * 0.5
    mask, face_id = mask.to(x.device), face_id.to(x.device)
    if tuple(mask.shape) != tuple(x.shape[:3]) or tuple(face_id.shape) != tuple(x.shape[:3]):
        raise ValueError(f"mask and face_id must be {list(x.shape[:3])}")
    edge = torch.zeros_like(mask, dtype=torch.bool)
    edge[:, :, :-1] |= face_id[:, :, :-1] != face_id[:, :, 1:]
    edge[:, :-1, :] |= face_id[:, :-1, :] != face_id[:, 1:, :]
    edge &= mask.bool()
    t = torch.tensor(tint, device=x.device, dtype=x.dtype)
    a = (mask.to(x.dtype) * alpha)[..., None]
    x = x * (1.0 - a) + t * a
    x = torch.where(edge[..., None], t.expand_as(x), x)
    strip = torch.cat(list(x), 1)  # [H, N W, 3]
    return (strip * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)


# ---- UV texture atlases (include/mvd.h: the conventions of the mvd_op_mesh_vertex_normals ... _render_uv block)
def read_mesh_uv(path):
    """(verts float64 [Nv,3], faces int32 [Nf,3], uv float64 [Nt,2], face_uv int32 [Nf,3]) of a Wavefront OBJ with texture
    coordinates: ``f`` lines in the v/vt and v/vt/vn forms, negative indices in both index sets, polygons fan-triangulated in both.
    ValueError if a face corner has no ``vt`` or an index is out of range."""
    path = str(path)
    if not path.lower().endswith(".obj"):
        raise ValueError(f"{path}: expected an .obj mesh with vt lines")
    vs, vts, tris, uvtris = [], [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                p = line.split()
                vs.append([float(p[1]), float(p[2]), float(p[3])])
            elif line.startswith("vt "):
                p = line.split()
                vts.append([float(p[1]), float(p[2])])
            elif line.startswith("f "):
                poly, uvpoly = [], []
                for tok in line.split()[1:]:
                    part = tok.split("/")
                    if len(part) < 2 or not part[1]:
                        raise ValueError(f"{path}: the face corner {tok!r} has no vt index")
                    i, t = int(part[0]), int(part[1])
                    poly.append(i - 1 if i > 0 else len(vs) + i)
                    uvpoly.append(t - 1 if t > 0 else len(vts) + t)
                if len(poly) < 3:
                    raise ValueError(f"{path}: a face with fewer than 3 vertices")
                _fan(poly, tris)
                _fan(uvpoly, uvtris)
    if not vs or not tris:
        raise ValueError(f"{path}: no vertices or no faces")
    verts, uv = np.asarray(vs, dtype=np.float64), np.asarray(vts, dtype=np.float64).reshape(-1, 2)
    faces, face_uv = np.asarray(tris, dtype=np.int64).reshape(-1, 3), np.asarray(uvtris, dtype=np.int64).reshape(-1, 3)
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f"{path}: a face index is outside the {len(verts)} vertices")
    if face_uv.min() < 0 or face_uv.max() >= len(uv):
        raise ValueError(f"{path}: a vt index is outside the {len(uv)} texture coordinates")
    return verts, faces.astype(np.int32), uv, face_uv.astype(np.int32)


def _atlas_size(size):
    Ht, Wt = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    if not (1 <= Ht <= 4096 and 1 <= Wt <= 4096):
        raise ValueError(f"the atlas must be 1..4096 texels on a side, got {(Ht, Wt)}")
    return Ht, Wt


def uv_to_atlas(uv, Ht, Wt):
    """Chart coordinates int32 [Nt,2] in 1/16 texel of uv [Nt,2] (OBJ convention: u right, v up, (0, 0) bottom-left) in an atlas of
    Ht x Wt texels with row 0 at the top: xs = rint(16 (u Wt - 0.5)), ys = rint(16 ((1 - v) Ht - 0.5)), float64 on the host.
    ValueError for a non-finite UV or one outside [0, 1]."""
    a = (uv.detach().cpu().numpy() if torch.is_tensor(uv) else np.asarray(uv)).astype(np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"uv must be [Nt,2], got {a.shape}")
    if not np.isfinite(a).all() or a.min() < 0.0 or a.max() > 1.0:
        raise ValueError("uv must be finite and inside [0, 1]")
    Ht, Wt = _atlas_size((Ht, Wt))
    xs = np.rint(16.0 * (a[:, 0] * Wt - 0.5))
    ys = np.rint(16.0 * ((1.0 - a[:, 1]) * Ht - 0.5))
    return np.stack([xs, ys], -1).astype(np.int32)


def triangle_atlas(n_faces, Ht, Wt, gutter=1):
    """(uv float64 [3 n_faces,2], face_uv int32 [n_faces,3]) of a deterministic atlas for a mesh without UVs: square cells of s
    texels in row-major order, two right triangles per cell (faces 2 c and 2 c + 1), every face with corners of its own.  In a
    cell's texel indices 0..s-1, with m = s - gutter and a = s - 2 gutter - 2, face 2 c owns the texels with i + j <= a and face
    2 c + 1 those with i, j <= m - 1 and i + j >= 2 (m - 1) - a (the chart corners sit a quarter texel outside those texel centres,
    on the 1/16 grid), so any two charts are more than ``gutter`` texels apart (Chebyshev).  s is the largest size at which
    the cells fit; ValueError when that leaves s < 2 gutter + 2, where a face would own no texel centre."""
    n_faces, gutter = int(n_faces), int(gutter)
    Ht, Wt = _atlas_size((Ht, Wt))
    if n_faces < 1 or gutter < 0:
        raise ValueError(f"triangle_atlas: needs n_faces >= 1 and gutter >= 0, got {n_faces}, {gutter}")
    cells = (n_faces + 1) // 2
    s = min(Ht, Wt)
    while s >= 1 and (Ht // s) * (Wt // s) < cells:
        s -= 1
    if s < 2 * gutter + 2:
        raise ValueError(f"triangle_atlas: {n_faces} faces in {Ht} x {Wt} texels leave cells of {s} texels; gutter {gutter} needs "
                         f"{2 * gutter + 2}")
    cols, m, a = Wt // s, s - gutter, s - 2 * gutter - 2
    f = np.arange(n_faces)
    x0, y0 = ((f // 2) % cols * s).astype(np.float64), ((f // 2) // cols * s).astype(np.float64)
    lo, hi = -0.25, a + 0.5
    first = np.array([[lo, lo], [hi, lo], [lo, hi]])                      # corners 0, 1, 2 of face 2 c: (x, y) in texel indices
    second = (m - 1.0) - first                                            # face 2 c + 1: the same triangle turned half way round
    local = np.where((f % 2 == 0)[:, None, None], first[None], second[None])
    x, y = local[..., 0] + x0[:, None], local[..., 1] + y0[:, None]
    uv = np.stack([(x + 0.5) / Wt, 1.0 - (y + 0.5) / Ht], -1).reshape(-1, 2)
    return uv, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def face_incidence(faces, Nv):
    """The vertex -> face incidence of a topology in CSR form: (inc_ptr int32 [Nv+1], inc_face int32 [3 Nf]); the faces of vertex v
    are inc_face[inc_ptr[v]:inc_ptr[v+1]], ascending (a face that names a vertex twice is listed twice, as the host
    vertex_normals adds it twice)."""
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1, 3)
    if len(f) < 1 or f.min() < 0 or f.max() >= Nv:
        raise ValueError(f"faces must be [Nf,3] with Nf >= 1 and indices inside [0, {Nv})")
    flat = f.reshape(-1)
    order = np.argsort(flat, kind="stable")
    ptr = np.zeros(Nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=Nv), out=ptr[1:])
    return ptr.astype(np.int32), (order // 3).astype(np.int32)


def vertex_normals_device(verts, faces, incidence=None):
    """Unit vertex normals on the device, float32, of verts [Nv,3] or a batch of frames [F,Nv,3] over one topology
    (mvd_op_mesh_vertex_normals): area-weighted as ``vertex_normals``, the faces of a vertex summed in ascending order without
    atomics, so frame f of a batch equals the frame computed alone.  ``incidence``: ``face_incidence(faces, Nv)`` kept by a caller
    that bakes many frames of one topology; by default the table is built here, on the host, at every call."""
    v = _as_tensor(verts, torch.float32)
    if v.dim() not in (2, 3) or v.shape[-1] != 3 or v.shape[-2] < 1:
        raise ValueError(f"verts must be [Nv,3] or [F,Nv,3], got {tuple(v.shape)}")
    single = v.dim() == 2
    vb = v[None] if single else v
    ptr, inc = face_incidence(faces, vb.shape[1]) if incidence is None else incidence
    dev = _device_of(verts)
    f = torch.from_numpy((faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int32).reshape(-1, 3))
    normals, bad = E.op_mesh_vertex_normals(vb, f, _as_tensor(ptr, torch.int32), _as_tensor(inc, torch.int32), device=dev)
    if int(bad.item()):
        raise ValueError(f"{int(bad.item())} entries of the incidence table were out of range")
    return normals[0] if single else normals


def _uv_args(uv, face_uv, Nf):
    a = (uv.detach().cpu().numpy() if torch.is_tensor(uv) else np.asarray(uv)).astype(np.float64)
    t = (face_uv.detach().cpu().numpy() if torch.is_tensor(face_uv) else np.asarray(face_uv)).astype(np.int64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"uv must be [Nt,2], got {a.shape}")
    if t.shape != (Nf, 3):
        raise ValueError(f"face_uv must be [{Nf},3], parallel to faces, got {t.shape}")
    if t.min() < 0 or t.max() >= len(a):
        raise ValueError(f"a face_uv index is outside the {len(a)} texture coordinates")
    return a, torch.from_numpy(t.astype(np.int32))


def _tex_face(uv_xy, face_uv, Ht, Wt, dev):
    tex_face, _, _ = E.op_mesh_raster(uv_xy[None], torch.ones((1, uv_xy.shape[0]), dtype=torch.int32), face_uv, Ht, Wt, device=dev)
    return tex_face[0]


def bake_texture(views, verts, faces, uv, face_uv, K, RT, size=1024, power=2.0, bias=4096, two_sided=False, fill=(0.5, 0.5, 0.5), pad=4,
                 z_near=None, incidence=None):
    """A UV texture atlas out of N views [N,3,H,W] or [N,H,W,3] (float in [-1, 1] or uint8) of the mesh (verts [Nv,3], faces
    [Nf,3]) with texture coordinates uv [Nt,2] / face_uv [Nf,3] under cameras K, RT; ``size``: texels on a side, or (Ht, Wt).
    Every texel centre inside a chart is lifted to its surface point, tested for visibility in every view with the integers of
    ``texture_mesh`` (the winning face must BE the texel's face, or the point lie within ``bias`` keys of the winner) and takes
    the mean of the view colours weighted by max(0, cos)^power.  Returns {"texture" [Ht,Wt,3] in [0, 1], row 0 at the top, after
    ``pad`` rounds of dilation into gutters and unseen texels (what stays invalid keeps ``fill``), "valid" [Ht,Wt] bool after
    the dilation, "tex_face" [Ht,Wt] int32 (-1: no chart), "n_seen", "weight_sum", "spread" [Ht,Wt] as texture_mesh defines them
    per vertex, "face_id", "mask" [N,H,W] of the views} (device tensors) and the floats "coverage" (share of the chart texels
    with a positive weight sum), "consistency" (mean spread where n_seen >= 2) and "z_near".  ``incidence``: ``face_incidence(faces, Nv)`` of the topology, for a
    caller that bakes many frames of it (default: built at every call, an argsort over 3 Nf entries on the host)."""
    if not torch.is_tensor(views):
        views = torch.as_tensor(np.asarray(views))
    if views.dim() != 4 or (views.shape[1] == 3) == (views.shape[3] == 3):
        raise ValueError(f"views must be [N,3,H,W] or [N,H,W,3], got {tuple(views.shape)}")
    N, H, W = (views.shape[0], views.shape[2], views.shape[3]) if views.shape[1] == 3 else tuple(views.shape[:3])
    v, f = _mesh_args(verts, faces)
    uv, face_uv = _uv_args(uv, face_uv, f.shape[0])
    Ht, Wt = _atlas_size(size)
    K3, RT = _cameras(K, RT)
    if K3.shape[0] != N:
        raise ValueError(f"{N} views but {K3.shape[0]} cameras")
    if not 0 <= int(pad) <= 64:
        raise ValueError(f"pad must be in 0..64, got {pad}")
    uv_xy = torch.from_numpy(uv_to_atlas(uv, Ht, Wt))  # refuses bad UVs before anything is launched
    z_near = default_z_near(v, RT) if z_near is None else float(z_near)
    dev = _device_of(views, verts, K)
    _, _, face_id, pix_key = _raster(v, f, K3, RT, H, W, z_near, dev)
    tex_face = _tex_face(uv_xy, face_uv, Ht, Wt, dev)
    normals = vertex_normals_device(v.to(dev), f, incidence=incidence)
    centres = -torch.einsum("nji,nj->ni", RT[:, :, :3], RT[:, :, 3])  # -R^T t
    out = E.op_mesh_texel_bake(views, face_id, pix_key, K3, RT, centres, z_near, v, normals, f, uv_xy, face_uv, tex_face, power=power,
                               bias=bias, two_sided=two_sided, fill=fill, taps=False, device=dev)
    seen = out["weight_sum"] > 0
    texture, valid = E.op_mesh_texture_dilate(out["texture"], seen, int(pad), device=dev)
    chart = tex_face >= 0
    multi = (out["n_seen"] >= 2) & ~torch.isnan(out["spread"])
    return {"texture": texture, "valid": valid, "tex_face": tex_face, "n_seen": out["n_seen"], "weight_sum": out["weight_sum"],
            "spread": out["spread"], "face_id": face_id, "mask": face_id >= 0, "z_near": z_near,
            "coverage": float((seen & chart).sum().double() / chart.sum().clamp(min=1).double()),
            "consistency": float(out["spread"][multi].double().mean()) if bool(multi.any()) else float("nan")}


def render_textured(texture, verts, faces, uv, face_uv, K, RT, H, W, background=(1.0, 1.0, 1.0), z_near=None):
    """The textured mesh in the N cameras K, RT at H x W with perspective-correct texture coordinates: {"images" [N,3,H,W] float32
    in [-1, 1] (the samplers' convention: feed it to ``image_metrics`` or ``texture_mesh``), "mask" [N,H,W] bool (covered),
    "face_id" [N,H,W] int32}.  texture [Ht,Wt,3] in [0, 1], row 0 at the top; bilinear, clamped to the edge; uncovered pixels
    take ``background`` (in [0, 1])."""
    v, f = _mesh_args(verts, faces)
    uv, face_uv = _uv_args(uv, face_uv, f.shape[0])
    if not torch.is_tensor(texture):
        texture = torch.as_tensor(np.asarray(texture))
    if texture.dim() != 3 or texture.shape[2] != 3 or not texture.is_floating_point():
        raise ValueError(f"texture must be a float tensor [Ht,Wt,3], got {texture.dtype} {tuple(texture.shape)}")
    _atlas_size(texture.shape[:2])
    if not np.isfinite(uv).all():
        raise ValueError("uv must be finite")
    K3, RT = _cameras(K, RT)
    z_near = default_z_near(v, RT) if z_near is None else float(z_near)
    dev = _device_of(texture, verts, K)
    xy, key, face_id, _ = _raster(v, f, K3, RT, int(H), int(W), z_near, dev)
    images = E.op_mesh_render_uv(xy, key, face_id, f, face_uv, torch.from_numpy(uv), texture, background=background, device=dev)
    return {"images": images, "mask": face_id >= 0, "face_id": face_id}


def reprojection_metrics(views, bake, verts, faces, uv, face_uv, K, RT, z_near=None):
    """How well a baked atlas explains the views it came from, no ground truth needed: ``bake["texture"]`` rendered back into
    the baking cameras and scored against ``views`` by ``metrics.image_metrics`` with the uncovered pixels as background
    (``mask=~mask``).  Returns image_metrics' dict plus "images" and "mask" of the render."""
    from .metrics import image_metrics
    if not torch.is_tensor(views):
        views = torch.as_tensor(np.asarray(views))
    if views.dim() != 4 or (views.shape[1] == 3) == (views.shape[3] == 3):
        raise ValueError(f"views must be [N,3,H,W] or [N,H,W,3], got {tuple(views.shape)}")
    H, W = (views.shape[2], views.shape[3]) if views.shape[1] == 3 else tuple(views.shape[1:3])
    r = render_textured(bake["texture"], verts, faces, uv, face_uv, K, RT, H, W, z_near=bake.get("z_near") if z_near is None else z_near)
    if r["images"].shape[0] != views.shape[0]:
        raise ValueError(f"{views.shape[0]} views but {r['images'].shape[0]} cameras")
    out = dict(image_metrics(r["images"], views.to(r["images"].device), mask=~r["mask"]))
    out["images"], out["mask"] = r["images"], r["mask"]
    return out


def write_obj(path, verts, faces, uv, face_uv, texture, texture_name=None):
    """A textured Wavefront OBJ: ``path`` (.obj) with ``v``, ``vt`` and ``f v/vt`` lines (17 significant digits: read_mesh_uv
    reads the same float64 back), beside it the .mtl of the same stem and the texture as a PNG, rint(255 c) of texture [Ht,Wt,3]
    in [0, 1] written as it is (row 0 at the top) -- ``texture_name``: its file name in the same folder, default <stem>.png.
    Returns the three paths."""
    import os
    from PIL import Image
    path = str(path)
    if not path.lower().endswith(".obj"):
        raise ValueError(f"{path}: expected an .obj path")
    v = (verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)).astype(np.float64)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1, 3)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts must be [Nv,3], got {v.shape}")
    a, t = _uv_args(uv, face_uv, len(f))
    t = t.numpy()
    tex = (texture.detach().cpu().numpy() if torch.is_tensor(texture) else np.asarray(texture)).astype(np.float64)
    if tex.ndim != 3 or tex.shape[2] != 3:
        raise ValueError(f"texture must be [Ht,Wt,3], got {tex.shape}")
    stem = path[:-4]
    folder, base = os.path.split(stem)
    png = texture_name or base + ".png"
    Image.fromarray(np.rint(np.clip(np.nan_to_num(tex), 0.0, 1.0) * 255.0).astype(np.uint8)).save(os.path.join(folder, png))
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl baked\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {png}\n")
    with open(path, "w") as fh:
        fh.write(f"mtllib {base}.mtl\n")
        fh.writelines(f"v {p[0]!r} {p[1]!r} {p[2]!r}\n" for p in v.tolist())
        fh.writelines(f"vt {p[0]!r} {p[1]!r}\n" for p in a.tolist())
        fh.write("usemtl baked\n")
        fh.writelines(f"f {i[0] + 1}/{j[0] + 1} {i[1] + 1}/{j[1] + 1} {i[2] + 1}/{j[2] + 1}\n" for i, j in zip(f.tolist(), t.tolist()))
    return {"obj": path, "mtl": stem + ".mtl", "png": os.path.join(folder, png)}


# ---- closest points and surface distances (include/mvd.h: mvd_op_mesh_closest_point)
def _cloud_faces(n):
    """A point cloud as a mesh: faces (i, i, i), whose closest point is the vertex itself."""
    return torch.arange(n, dtype=torch.int32)[:, None].expand(n, 3).contiguous()


def _points_arg(name, a):
    t = _as_tensor(a, torch.float32)
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{name} must be [n,3] with n >= 1, got {tuple(t.shape)}")
    return t


def closest_point(points, verts, faces, normals=None, cos_min=None, max_dist=None):
    """For every point [Q,3] the closest point of the mesh verts [Nv,3] / faces [Nf,3] (``faces=None``: verts is a point cloud), by
    exhaustive search on the device (mvd_op_mesh_closest_point: exact, smallest distance, ties to the smallest face index).
    ``normals`` [Q,3] with ``cos_min`` (default 0) admits only faces whose normal makes a cosine >= cos_min with the point's; beyond
    ``max_dist`` a point has no match.  Returns a dict of device tensors: face [Q] int32 (-1: no match), bary [Q,3], point [Q,3],
    dist2 [Q], dist [Q] (+inf: no match), matched [Q] bool."""
    pts, v = _points_arg("points", points), _points_arg("verts", verts)
    if faces is None:
        f = _cloud_faces(v.shape[0])
    else:
        _, f = _mesh_args(v, faces)
    if cos_min is not None and normals is None:
        raise ValueError("cos_min needs the points' normals")
    nrm = None
    if normals is not None:
        nrm = _points_arg("normals", normals)
        if nrm.shape[0] != pts.shape[0]:
            raise ValueError(f"normals must be [{pts.shape[0]},3], got {tuple(nrm.shape)}")
    cos_min = 0.0 if cos_min is None else float(cos_min)
    if not -1.0 <= cos_min <= 1.0:
        raise ValueError(f"cos_min must be in [-1, 1], got {cos_min}")
    if max_dist is not None and not float(max_dist) > 0.0:
        raise ValueError(f"max_dist must be positive, got {max_dist}")
    # the gate compares float32 squares: the float32 nearest to max_dist^2
    max_dist2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
    out = E.op_mesh_closest_point(pts, v, f, query_normals=nrm, cos_min=cos_min, max_dist2=max_dist2, device=_device_of(points, verts))
    out.pop("key")
    out["dist"] = out["dist2"].sqrt()
    out["matched"] = out["face"] >= 0
    return out


def _quantile(sorted_values, q):
    """numpy.percentile's default (linear interpolation between order statistics) of an ascending float64 tensor."""
    pos = q * (sorted_values.numel() - 1)
    lo = int(pos)
    hi = min(lo + 1, sorted_values.numel() - 1)
    return float(sorted_values[lo] + (sorted_values[hi] - sorted_values[lo]) * (pos - lo))


def distance_statistics(dist):
    """mean / rms / median / p90 / max of the finite entries of dist (float64 on its device) and their share ``matched``; NaN
    statistics when no entry is finite."""
    d = dist.double()
    ok = torch.isfinite(d)
    d = d[ok].sort().values
    n = d.numel()
    if n == 0:
        nan = float("nan")
        return {"mean": nan, "rms": nan, "median": nan, "p90": nan, "max": nan, "matched": 0.0}
    return {"mean": float(d.mean()), "rms": float((d * d).mean().sqrt()), "median": _quantile(d, 0.5), "p90": _quantile(d, 0.9),
            "max": float(d[-1]), "matched": n / dist.numel()}


def surface_distance(points, verts, faces, normals=None, cos_min=None, max_dist=None, symmetric=False, point_faces=None):
    """Distance of every point [Q,3] to the mesh verts / faces (``closest_point``) and its statistics over the matched points:
    {"dist" [Q] (device, +inf: no match), "mean", "rms", "median", "p90", "max", "matched" (their share)}.  With a scan's vertices as
    ``points`` and the posed model as the mesh this is the scan-to-mesh distance of the 3-D benchmarks.  ``symmetric``: adds
    "back", the same dict for the mesh's vertices against the points (as a surface with ``point_faces``, else as a cloud; no
    normal gate in that direction), and "chamfer", the mean of the two means."""
    fwd = closest_point(points, verts, faces, normals=normals, cos_min=cos_min, max_dist=max_dist)
    out = dict(distance_statistics(fwd["dist"]), dist=fwd["dist"])
    if symmetric:
        back = closest_point(verts, points, point_faces, max_dist=max_dist)
        out["back"] = dict(distance_statistics(back["dist"]), dist=back["dist"])
        out["chamfer"] = 0.5 * (out["mean"] + out["back"]["mean"])
    return out
