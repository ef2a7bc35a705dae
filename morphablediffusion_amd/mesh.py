"""A coloured mesh out of generated views (include/mvd.h: mvd_op_mesh_project / _raster / _vertex_colors, csrc/k_mesh.hip): the
conditioning mesh is rasterised into the N target cameras with exact integer visibility, and each vertex takes the weighted mean
of the view colours that see it.  Not a reference feature (its only 3-D output is a NeuS2 data folder).

  read_mesh         vertices and triangles of an OBJ / PLY file          vertex_normals   area-weighted, host, float64
  rasterize_mesh    face_id / pix_key / depth / mask of every view       texture_mesh     per-vertex colours and their statistics
  write_ply         binary little-endian, uchar colours                  overlay_views    the mesh drawn over the views (plain torch)

What is exact: everything after the projection (coverage, depth order, visibility, n_seen) is integer arithmetic.  What is not
computed: UV texture maps, perspective-correct attribute rendering, the input photo as a 17th view (its camera is not in the
batch).  The FLAME mesh ends at the head, so colour on hair and shoulders is not recovered."""
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
