"""The morphable-model forward: FLAME / SMPL-X parameters to vertices on the device (csrc/k_morph.hip through engine.op_morph_*).

The reference conditions on a mesh file that a second program writes: MICA's ``FLAME`` module (third_party/MICA/models/flame.py,
lbs.py) turns shape, expression and pose parameters into 5023 vertices.  ``MorphableModel`` is that step: it loads the model
arrays (an ``.npz`` or the licensed ``.pkl`` with the same key names), folds the joint regressor into the template and the shape
directions, re-packs the blend shapes to one [L,3V] basis, and runs linear blend skinning for one frame or a sweep of them.  The
vertices go straight into ``batch.build_batch`` / ``stack_batches`` / ``model.sample`` / ``mesh.texture_mesh`` / ``write_ply``.

    fm = MorphableModel.load("flame.npz", n_shape=300, n_exp=100)
    out = fm.flame(shape, expression=exp, jaw=jaw, post=flame_alignment())
    batch = frames_to_batch(input_image, out["vertices"], device="cuda:0")

Units: FLAME's forward is in metres, and so are the mesh files of the reference pipeline, so ``unit_scale``
defaults to 1.0.  The inverse is here too (csrc/k_morph_bwd.hip): ``vjp`` is the vector-Jacobian product of the forward,
``differentiable`` the same as a torch.autograd.Function, ``fit`` / ``fit_flame`` run Adam on the device against target vertices
and 3-D landmarks, ``fit_scan`` / ``fit_flame_scan`` against a scan of any topology (closest points, csrc/k_closest.hip),
``fit_2d`` / ``fit_flame_2d`` against 2-D key points in calibrated views, with the pose-dependent contour landmarks chosen per view
(csrc/k_morph_2d.hip).  Not here: a landmark detector (vertex normals of a batch of frames: mesh.vertex_normals_device).

    fit = fm.fit_flame(target_vertices=mesh_vertices, free=("expression", "jaw"), prior={"shape": mica_shape})
"""
import io
import pickle
from typing import Dict, Optional

import numpy as np
import torch

from . import batch as B
from . import engine as E

FLAME_EXPRESSION_OFFSET = 300  # FLAME's shapedirs: identity in columns 0..299, expression from column 300 on (flame.py:68)
FLAME_JOINTS = ("global", "neck", "jaw", "eye_left", "eye_right")
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights", "f")
LANDMARK_KEYS = ("static_lmk_faces_idx", "static_lmk_bary_coords")  # optional, the names of FLAME's landmark embedding
CONTOUR_KEYS = ("dynamic_lmk_faces_idx", "dynamic_lmk_bary_coords")  # optional: the per-view contour table [R,Md] / [R,Md,3]
FLAME_NECK_JOINT = 1


class _ChumpyArray:
    """Stand-in for every ``chumpy.*`` class of a model pickle: keeps the pickled state, whose ``x`` is the array."""

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {"x": state})

    def array(self):
        if "x" in self.__dict__:
            return np.asarray(self.__dict__["x"])
        for v in self.__dict__.values():
            if isinstance(v, np.ndarray):
                return v
        raise pickle.UnpicklingError("a chumpy object of the model file holds no array")


_NUMPY_GLOBALS = {(m, n) for m in ("numpy.core.multiarray", "numpy._core.multiarray") for n in ("_reconstruct", "scalar")} | \
    {("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}
# object construction without a constructor call (protocols 0 and 1), and the str -> bytes step of arrays that Python 3 wrote at
# protocol 2 or below
_PLAIN_GLOBALS = {("copyreg", "_reconstructor"), ("copy_reg", "_reconstructor"), ("builtins", "object"), ("__builtin__", "object"),
                  ("_codecs", "encode")}
_SCIPY_CLASSES = {"csc_matrix", "csr_matrix", "coo_matrix", "csc_array", "csr_array", "coo_array"}


class RestrictedUnpickler(pickle.Unpickler):
    """Reads a FLAME / SMPL-X model pickle and nothing else: numpy array reconstruction, a scipy sparse matrix if scipy imports,
    ``chumpy.*`` as a stand-in that keeps the array (chumpy itself is not needed); any other global raises UnpicklingError."""

    def find_class(self, module, name):
        if (module, name) in _NUMPY_GLOBALS or (module, name) in _PLAIN_GLOBALS:
            return super().find_class(module, name)
        if module == "chumpy" or module.startswith("chumpy."):
            return _ChumpyArray
        if module.startswith("scipy.sparse") and name in _SCIPY_CLASSES:
            try:
                import scipy.sparse  # noqa: F401
            except ImportError:
                raise pickle.UnpicklingError(f"the model file holds a {module}.{name}, and scipy is not installed")
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"global {module}.{name} is not allowed in a morphable-model file")


def _plain(v):
    """A value of a model file as a numpy array: chumpy stand-ins and sparse matrices unwrapped."""
    if isinstance(v, _ChumpyArray):
        v = v.array()
    if hasattr(v, "toarray") and not isinstance(v, np.ndarray):
        v = v.toarray()
    return np.asarray(v)


def read_model_file(path) -> Dict[str, np.ndarray]:
    """{key: array} of an ``.npz`` (read without pickle) or a ``.pkl`` (through RestrictedUnpickler, latin1 as the Python 2
    pickles need) with the FLAME / SMPL-X key names; only the keys the forward needs are returned."""
    path = str(path)
    if path.lower().endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
    elif path.lower().endswith(".pkl"):
        with open(path, "rb") as f:
            d = RestrictedUnpickler(io.BytesIO(f.read()), encoding="latin1").load()
        if not isinstance(d, dict):
            raise ValueError(f"{path}: expected a pickled dict of model arrays")
    else:
        raise ValueError(f"{path}: expected a .npz or .pkl model file")
    missing = [k for k in MODEL_KEYS[:-1] if k not in d]
    if missing:
        raise ValueError(f"{path}: missing {missing}")
    return {k: _plain(d[k]) for k in MODEL_KEYS + LANDMARK_KEYS + CONTOUR_KEYS if k in d}


def _rows(x, F, width, name):
    """x as a float64 [F,width] array; a vector is one row, one row is repeated for every frame, None is zeros."""
    if x is None:
        return np.zeros((F, width))
    x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    if x.ndim != 2 or x.shape[1] != width or x.shape[0] not in (1, F):
        raise ValueError(f"{name} must be [{width}] or [F,{width}] with F = {F}, got {x.shape}")
    return np.broadcast_to(x, (F, width))


class MorphableModel:
    """A linear-blend-skinning model on one device: v_template [V,3], basis [L,3V] (shape directions, then pose directions),
    weights [V,J], the folded joint regressor (j_template [J,3], j_dirs [NB,3J]) and the host list ``parents``."""

    def __init__(self):
        raise TypeError("use MorphableModel.from_arrays or MorphableModel.load")

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, parents, weights, faces=None, lmk_face=None, lmk_bary=None,
                    device="cuda:0", unit_scale=1.0, n_shape=None, dyn_lmk_face=None, dyn_lmk_bary=None, neck_joint=None):
        """v_template [V,3], shapedirs [V,3,NB], posedirs [V,3,9 (J-1)] (the pickle's layout) or [9 (J-1),3V] (lbs.py's),
        J_regressor [J,V] (dense or scipy sparse), parents [J] (parents[0] is taken as the root whatever it holds), weights [V,J];
        optional faces [Nf,3] and a static landmark embedding lmk_face [M], lmk_bary [M,3].  The folds run in float64:
        j_template = J_regressor v_template, j_dirs = J_regressor shapedirs, basis = [shapedirs^T; posedirs]; lengths are
        multiplied by unit_scale; the device gets float32.  n_shape: how many leading betas ``flame`` takes as identity.
        dyn_lmk_face [R,Md], dyn_lmk_bary [R,Md,3] (R odd; FLAME: 79 x 17) and neck_joint (default 1, FLAME's neck; 0 with one
        joint): the contour landmarks, whose row is chosen per view from the head's yaw in that view (fit_2d)."""
        who = "MorphableModel.from_arrays"
        vt = _plain(v_template).astype(np.float64)
        if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise ValueError(f"{who}: v_template must be [V,3], got {vt.shape}")
        V = vt.shape[0]
        S = _plain(shapedirs).astype(np.float64)
        if S.ndim != 3 or S.shape[:2] != (V, 3) or S.shape[2] < 1:
            raise ValueError(f"{who}: shapedirs must be [V,3,NB] with V = {V}, got {S.shape}")
        NB = S.shape[2]
        Jr = _plain(J_regressor).astype(np.float64)
        if Jr.ndim != 2 or Jr.shape[1] != V or Jr.shape[0] < 1:
            raise ValueError(f"{who}: J_regressor must be [J,V] with V = {V}, got {Jr.shape}")
        J = Jr.shape[0]
        if J > E.MORPH_MAX_JOINTS:
            raise ValueError(f"{who}: at most {E.MORPH_MAX_JOINTS} joints, got {J}")
        par = [int(p) for p in np.asarray(_plain(parents)).reshape(-1).astype(np.int64)]
        if par:
            par[0] = -1  # kintree_table stores 2^32 - 1 there (flame.py:82-83)
        par = E.morph_parents(who, par, J)
        W = _plain(weights).astype(np.float64)
        if W.shape != (V, J):
            raise ValueError(f"{who}: weights must be [V,J] = [{V},{J}], got {W.shape}")
        P = _plain(posedirs).astype(np.float64)
        NP = 9 * (J - 1)
        if P.ndim == 3 and P.shape == (V, 3, NP):
            P = P.reshape(3 * V, NP).T
        elif P.ndim != 2 or P.shape != (NP, 3 * V):
            raise ValueError(f"{who}: posedirs must be [V,3,{NP}] or [{NP},{3 * V}], got {P.shape}")
        s = float(unit_scale)
        self = object.__new__(cls)
        self.V, self.NB, self.J, self.parents, self.unit_scale = V, NB, J, par, s
        self.n_shape = NB if n_shape is None else int(n_shape)
        if not 0 <= self.n_shape <= NB:
            raise ValueError(f"{who}: n_shape must be in 0..{NB}, got {n_shape}")
        self.device = torch.device(device)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.v_template = f32(vt * s)
        self.basis = f32(np.concatenate([S.reshape(3 * V, NB).T, P], 0) * s)
        self.weights = f32(W)
        self.j_template = f32(Jr @ vt * s)
        self.j_dirs = f32(np.einsum("jv,vkn->njk", Jr, S).reshape(NB, 3 * J) * s)
        self.faces = self.lmk_face = self.lmk_bary = self.csr_ptr = self.csr_ent = None
        if faces is not None:
            fc = np.asarray(_plain(faces)).astype(np.int64)
            if fc.ndim != 2 or fc.shape[1] != 3 or fc.shape[0] < 1 or fc.min() < 0 or fc.max() >= V:
                raise ValueError(f"{who}: faces must be [Nf,3] with indices in 0..{V - 1}, got {fc.shape}")
            self.faces = torch.from_numpy(fc.astype(np.int32)).to(self.device)
        if (lmk_face is None) != (lmk_bary is None):
            raise ValueError(f"{who}: lmk_face and lmk_bary go together")
        if lmk_face is not None:
            if self.faces is None:
                raise ValueError(f"{who}: a landmark embedding needs faces")
            lf, lb = np.asarray(_plain(lmk_face)).astype(np.int64).reshape(-1), _plain(lmk_bary).astype(np.float64)
            if len(lf) < 1 or lb.shape != (len(lf), 3) or lf.min() < 0 or lf.max() >= self.faces.shape[0]:
                raise ValueError(f"{who}: lmk_face must be [M] face indices and lmk_bary [M,3], got {lf.shape} and {lb.shape}")
            self.lmk_face, self.lmk_bary = torch.from_numpy(lf.astype(np.int32)).to(self.device), f32(lb)
            # the backward of the landmarks is a gather through this table: entries ascending, no atomics
            self.csr_ptr, self.csr_ent = (torch.from_numpy(a).to(self.device) for a in E.landmark_csr(fc, lf, lb, V))
        self.dyn_lmk_face = self.dyn_lmk_bary = self.ct_vert = self.ct_ptr = self.ct_ent = None
        self.neck_joint = min(FLAME_NECK_JOINT, J - 1) if neck_joint is None else int(neck_joint)
        if not 0 <= self.neck_joint < J:
            raise ValueError(f"{who}: neck_joint must be in 0..{J - 1}, got {neck_joint}")
        if (dyn_lmk_face is None) != (dyn_lmk_bary is None):
            raise ValueError(f"{who}: dyn_lmk_face and dyn_lmk_bary go together")
        if dyn_lmk_face is not None:
            if self.faces is None:
                raise ValueError(f"{who}: a contour embedding needs faces")
            df, db = np.asarray(_plain(dyn_lmk_face)).astype(np.int64), _plain(dyn_lmk_bary).astype(np.float64)
            if df.ndim != 2 or df.shape[0] % 2 != 1 or df.shape[1] < 1 or db.shape != df.shape + (3,):
                raise ValueError(f"{who}: dyn_lmk_face must be [R,Md] with R odd and dyn_lmk_bary [R,Md,3], got {df.shape} and {db.shape}")
            table = E.contour_table(fc, df, V)  # a face index outside the mesh gives NaN landmarks and no entry
            if table[0].size == 0:
                raise ValueError(f"{who}: no face of dyn_lmk_face is a face of the mesh")
            self.dyn_lmk_face, self.dyn_lmk_bary = torch.from_numpy(np.ascontiguousarray(df, dtype=np.int32)).to(self.device), f32(db)
            # the backward of the contour landmarks is a gather through this table, as the static landmarks' is
            self.ct_vert, self.ct_ptr, self.ct_ent = (torch.from_numpy(a).to(self.device) for a in table)
        return self

    @classmethod
    def load(cls, path, n_shape=None, n_exp=None, device="cuda:0", unit_scale=1.0):
        """A model file (read_model_file).  n_shape / n_exp select columns of shapedirs as the reference's FLAME.__init__ does:
        the first n_shape, then those from column 300 on (the first n_exp of them if n_exp is given); with neither, every
        column is kept."""
        d = read_model_file(path)
        S = d["shapedirs"]
        if S.ndim != 3:
            raise ValueError(f"{path}: shapedirs must be [V,3,NB], got {S.shape}")
        if n_shape is not None or n_exp is not None:
            ns = min(FLAME_EXPRESSION_OFFSET, S.shape[2]) if n_shape is None else int(n_shape)
            exp = S[:, :, FLAME_EXPRESSION_OFFSET:]
            ne = exp.shape[2] if n_exp is None else int(n_exp)
            if not (0 <= ns <= S.shape[2]) or not (0 <= ne <= exp.shape[2]) or ns + ne < 1:
                raise ValueError(f"{path}: shapedirs has {S.shape[2]} columns ({exp.shape[2]} from column {FLAME_EXPRESSION_OFFSET} "
                                 f"on), cannot take n_shape = {n_shape}, n_exp = {n_exp}")
            S, n_shape = np.concatenate([S[:, :, :ns], exp[:, :, :ne]], 2), ns
        kt = np.asarray(d["kintree_table"])
        lm = {"lmk_face": d.get(LANDMARK_KEYS[0]), "lmk_bary": d.get(LANDMARK_KEYS[1])}
        if d.get("f") is not None and all(k in d for k in CONTOUR_KEYS):
            lm.update(dyn_lmk_face=d[CONTOUR_KEYS[0]], dyn_lmk_bary=d[CONTOUR_KEYS[1]])
        return cls.from_arrays(d["v_template"], S, d["posedirs"], d["J_regressor"], kt[0] if kt.ndim == 2 else kt, d["weights"],
                               faces=d.get("f"), device=device, unit_scale=unit_scale, n_shape=n_shape, **lm)

    def _params(self, who, betas, pose, transl=None):
        """(betas [F,NB], pose [F,J,3], transl [F,3] or None) as float32 tensors on the model's device, shapes checked."""
        if self.device.type != "cuda":
            raise ValueError(f"{who}: the model is on {self.device}; the forward runs on the GPU only (model.to('cuda:0'))")
        if not torch.is_tensor(betas) or not torch.is_tensor(pose):
            betas, pose = torch.as_tensor(np.asarray(betas)), torch.as_tensor(np.asarray(pose))
        if betas.dim() != 2 or betas.shape[1] != self.NB:
            raise ValueError(f"{who}: betas must be [F,{self.NB}], got {tuple(betas.shape)}")
        F = betas.shape[0]
        if pose.dim() == 2 and pose.shape == (F, 3 * self.J):
            pose = pose.reshape(F, self.J, 3)
        if tuple(pose.shape) != (F, self.J, 3):
            raise ValueError(f"{who}: pose must be [F,{self.J},3] or [F,{3 * self.J}] with F = {F}, got {tuple(pose.shape)}")
        if transl is not None:
            transl = transl if torch.is_tensor(transl) else torch.as_tensor(np.asarray(transl))
            transl = transl.reshape(1, 3).expand(F, 3) if transl.dim() == 1 and transl.numel() == 3 else transl
            if tuple(transl.shape) != (F, 3):
                raise ValueError(f"{who}: transl must be [3] or [F,3] with F = {F}, got {tuple(transl.shape)}")
        f32 = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        return f32(betas), f32(pose), f32(transl)

    def _run(self, betas, pose, post, transl, want_blend):
        """The three forward launches on checked parameters; with want_blend what the backward needs is kept."""
        dev = self.device
        p = E.op_morph_pose(betas, pose, self.j_template, self.j_dirs, self.parents, device=dev)
        coef = torch.cat([betas, p["pose_feature"]], 1) if self.J > 1 else betas
        blend = None
        if transl is None and not want_blend:  # what the forward has always launched
            verts = E.op_morph_skin(self.basis, self.v_template, coef, self.weights, p["A"], post=post, n_betas=self.NB, device=dev)
        else:
            r = E.op_morph_skin_ex(self.basis, self.v_template, coef, self.weights, p["A"], post=post, transl=transl, n_betas=self.NB,
                                   want_blend=want_blend, device=dev)
            verts, blend = r if want_blend else (r, None)
        lmk = None if self.lmk_face is None else E.op_morph_landmarks(verts, self.faces, self.lmk_face, self.lmk_bary, device=dev)
        return {"vertices": verts, "joints": p["joints"], "landmarks": lmk, "pose": pose, "j_rest": p["j_rest"], "A": p["A"],
                "blend": blend}

    def forward(self, betas, pose, post=None, transl=None) -> Dict[str, Optional[torch.Tensor]]:
        """betas [F,NB], pose [F,J,3] or [F,3J] (axis-angle), post [3,4] or None: an affine applied to the vertices in the
        skinning pass (flame_alignment()); transl [F,3] or [3] or None: a translation in the model's frame, added before post.
        Returns device tensors: vertices [F,V,3], joints [F,J,3] (the posed joints, in the model's frame: neither transl nor post
        is applied to them), landmarks [F,M,3] (of the returned vertices) or None without an embedding."""
        betas, pose, transl = self._params("MorphableModel.forward", betas, pose, transl)
        r = self._run(betas, pose, post, transl, False)
        return {k: r[k] for k in ("vertices", "joints", "landmarks")}

    def _backward(self, saved, post, grad_vertices, grad_joints, grad_landmarks):
        """The backward launches on what _run(..., want_blend=True) kept: {"betas", "pose", "transl"} gradients."""
        who, dev = "MorphableModel.vjp", self.device
        F = saved["pose"].shape[0]
        for name, g, shape in (("grad_vertices", grad_vertices, (F, self.V, 3)), ("grad_joints", grad_joints, (F, self.J, 3))):
            if g is not None and (not torch.is_tensor(g) or tuple(g.shape) != shape):
                raise ValueError(f"{who}: {name} must be a tensor {list(shape)}, got {tuple(getattr(g, 'shape', ()))}")
        g_y = grad_vertices
        if grad_landmarks is not None:
            if self.csr_ptr is None:
                raise ValueError(f"{who}: grad_landmarks given, and the model has no landmark embedding")
            g_y = E.op_morph_landmarks_bwd(grad_landmarks, self.csr_ptr, self.csr_ent, self.lmk_bary, self.V, g_in=g_y, device=dev)
        if g_y is None:
            if grad_joints is None:
                raise ValueError(f"{who}: give at least one of grad_vertices, grad_joints, grad_landmarks")
            g_y = torch.zeros((F, self.V, 3), device=dev)
        sb = E.op_morph_skin_bwd(g_y, self.weights, saved["A"], saved["blend"], self.basis, post=post, n_betas=self.NB, device=dev)
        return E.op_morph_pose_bwd(saved["pose"], saved["j_rest"], saved["A"], self.j_dirs, self.parents, sb["part_a"], sb["part_c"],
                                   g_joints=grad_joints, device=dev)

    def vjp(self, betas, pose, grad_vertices=None, grad_joints=None, grad_landmarks=None, post=None, transl=None):
        """The vector-Jacobian product of ``forward`` at (betas, pose, transl): the cotangents grad_vertices [F,V,3], grad_joints
        [F,J,3] and grad_landmarks [F,M,3] (any of them None) pulled back to {"betas" [F,NB], "pose" [F,J,3], "transl" [F,3]}."""
        betas, pose, transl = self._params("MorphableModel.vjp", betas, pose, transl)
        return self._backward(self._run(betas, pose, post, transl, True), post, grad_vertices, grad_joints, grad_landmarks)

    def differentiable(self, betas, pose, post=None, transl=None):
        """``forward`` as a torch.autograd.Function over the same kernels: betas, pose and transl may require gradients, and the
        returned vertices, joints and landmarks carry them, so a loss of one's own (a 2-D reprojection term, say) can be written
        in torch.  Float32 on the model's device; ``.backward()`` runs the launches of ``vjp``."""
        who = "MorphableModel.differentiable"
        if not all(torch.is_tensor(t) for t in (betas, pose)) or (transl is not None and not torch.is_tensor(transl)):
            raise ValueError(f"{who}: betas, pose and transl must be tensors")
        self._params(who, betas, pose, transl)  # the shape errors, before autograd sees anything
        F = betas.shape[0]
        has_t = transl is not None
        t_in = transl if has_t else torch.zeros((F, 3), device=self.device)
        out = _MorphFunction.apply(self, post, has_t, betas, pose, t_in)
        return {"vertices": out[0], "joints": out[1], "landmarks": out[2] if self.lmk_face is not None else None}

    # ---- fitting: Adam on the device against target vertices and 3-D landmarks (engine.morph_fit_run)
    def param_groups(self):
        """{name: slice} of the parameter row [betas | pose | transl] (P = NB + 3 J + 3 columns); a FLAME model adds the names of
        ``flame``'s arguments."""
        NB, J = self.NB, self.J
        g = {"betas": slice(0, NB), "pose": slice(NB, NB + 3 * J), "transl": slice(NB + 3 * J, NB + 3 * J + 3)}
        if J == len(FLAME_JOINTS):
            g.update({"shape": slice(0, self.n_shape), "expression": slice(self.n_shape, NB), "global_pose": slice(NB, NB + 3),
                      "neck": slice(NB + 3, NB + 6), "jaw": slice(NB + 6, NB + 9), "eyes": slice(NB + 9, NB + 15)})
        return g

    def fit_vectors(self, lr=0.05, free=None, reg=None, prior=None, fit_transl=True, who="MorphableModel.fit"):
        """The optimiser's per-parameter vectors (float64 numpy, [P] each): lr (0 = frozen), lam and p0 of the penalty
        lam (p - p0)^2.  free: None (everything) or names of param_groups(); reg: {name: lam}; prior: {name: vector}.
        fit_transl=False freezes the translation whatever ``free`` says."""
        groups = self.param_groups()
        P = self.NB + 3 * self.J + 3

        def sl(kind, name):
            if name not in groups:
                raise ValueError(f"{who}: {kind} names {name!r}; this model has {sorted(groups)}")
            return groups[name]

        lr = float(lr)
        if not (0.0 < lr < float("inf")):
            raise ValueError(f"{who}: lr must be positive and finite, got {lr}")
        lrv, lam, p0 = np.zeros(P), np.zeros(P), np.zeros(P)
        if free is None:
            lrv[:] = lr
        else:
            if isinstance(free, str):
                raise ValueError(f"{who}: free must be a sequence of names, not the string {free!r}")
            for name in free:
                lrv[sl("free", name)] = lr
        if not fit_transl:
            lrv[groups["transl"]] = 0.0
        if not lrv.any():
            raise ValueError(f"{who}: nothing is free")
        for name, val in (reg or {}).items():
            val = float(val)
            if not (0.0 <= val < float("inf")):
                raise ValueError(f"{who}: reg[{name!r}] must be non-negative and finite, got {val}")
            lam[sl("reg", name)] = val
        for name, vec in (prior or {}).items():
            s = sl("prior", name)
            vec = np.asarray(vec.detach().cpu() if torch.is_tensor(vec) else vec, dtype=np.float64).reshape(-1)
            if vec.shape[0] != s.stop - s.start:
                raise ValueError(f"{who}: prior[{name!r}] must have {s.stop - s.start} entries, got {vec.shape[0]}")
            p0[s] = vec
        return lrv, lam, p0

    def _fit_init(self, who, init, F, p0, lrv):
        """The start [F,P] (float64 numpy): zeros, a frozen column at its prior, then what ``init`` names."""
        groups = self.param_groups()
        p = np.zeros((F, p0.shape[0]))
        p[:, lrv == 0.0] = p0[lrv == 0.0]
        for name, val in (init or {}).items():
            if name not in groups:
                raise ValueError(f"{who}: init names {name!r}; this model has {sorted(groups)}")
            if val is not None:
                s = groups[name]
                p[:, s] = _rows(val.reshape(val.shape[0], -1) if np.ndim(val) == 3 else val, F, s.stop - s.start, f"init[{name!r}]")
        return p

    def fit(self, target_vertices=None, target_landmarks=None, vertex_weight=None, landmark_weight=None, lmk_lambda=1.0, iters=300,
            lr=0.05, init=None, free=None, reg=None, prior=None, post=None, fit_transl=True, _who="MorphableModel.fit"):
        """Adam on the device: parameters whose forward meets target_vertices [F,V,3] and / or target_landmarks [F,M,3] (3-D).
        Per frame E_f = sum_v w_v |y - t|^2 / sum_v w_v + lmk_lambda sum_m w'_m |l - l'|^2 / sum_m w'_m + sum_p lam_p (p - p0_p)^2;
        frames are independent.  init: {name: value} (zeros otherwise); free / reg / prior: see fit_vectors.  Returns device
        tensors: betas [F,NB], pose [F,J,3], transl [F,3], vertices [F,V,3] (of the fitted parameters), loss_history [iters,F]
        (the data term before each step) and rms [F]: the root mean square vertex distance to target_vertices, or to the target
        landmarks without them."""
        who = _who
        lrv, lam, p0 = self.fit_vectors(lr, free, reg, prior, fit_transl, who)
        if target_vertices is None and target_landmarks is None:
            raise ValueError(f"{who}: give target_vertices, target_landmarks or both")
        tv, tl = (None if t is None else (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))) for t in
                  (target_vertices, target_landmarks))
        tv = tv[None] if tv is not None and tv.dim() == 2 else tv
        tl = tl[None] if tl is not None and tl.dim() == 2 else tl
        if tv is not None and (tv.dim() != 3 or tuple(tv.shape[1:]) != (self.V, 3) or tv.shape[0] < 1):
            raise ValueError(f"{who}: target_vertices must be [F,{self.V},3] (the model's topology), got {tuple(tv.shape)}")
        if tl is not None:
            if self.lmk_face is None:
                raise ValueError(f"{who}: target_landmarks given, and the model has no landmark embedding")
            M = self.lmk_face.shape[0]
            if tl.dim() != 3 or tuple(tl.shape[1:]) != (M, 3) or tl.shape[0] < 1:
                raise ValueError(f"{who}: target_landmarks must be [F,{M},3], got {tuple(tl.shape)}")
        F = max(t.shape[0] for t in (tv, tl) if t is not None)
        if any(t is not None and t.shape[0] not in (1, F) for t in (tv, tl)):
            raise ValueError(f"{who}: target_vertices and target_landmarks must have the same number of frames (or one)")
        iters = int(iters)
        if iters < 1:
            raise ValueError(f"{who}: iters must be at least 1, got {iters}")
        start = self._fit_init(who, init, F, p0, lrv)
        if self.device.type != "cuda":
            raise ValueError(f"{who}: the model is on {self.device}; the fitter runs on the GPU only (model.to('cuda:0'))")
        dev = self.device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        p = f32(start)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        hist = E.morph_fit_run(self, p, m, v, f32(lrv), f32(lam), f32(p0), iters, target=tv, vertex_weight=vertex_weight, target_lmk=tl,
                               lmk_weight=landmark_weight, lmk_lambda=lmk_lambda, post=post)
        NB, J = self.NB, self.J
        out = {"betas": p[:, :NB].contiguous(), "pose": p[:, NB:NB + 3 * J].reshape(F, J, 3).contiguous(),
               "transl": p[:, NB + 3 * J:].contiguous(), "loss_history": hist}
        fw = self.forward(out["betas"], out["pose"], post=post, transl=out["transl"])
        out["vertices"] = fw["vertices"]
        got, want = (fw["vertices"], tv) if tv is not None else (fw["landmarks"], tl)
        out["rms"] = (got - want.to(device=dev, dtype=torch.float32)).square().sum(-1).mean(-1).sqrt()
        return out

    def fit_flame(self, target_vertices=None, target_landmarks=None, free=None, reg=None, prior=None, init=None, **kw):
        """``fit`` in ``flame``'s names: free=("expression", "jaw"), reg={"shape": 1e-4, "expression": 1e-4, "jaw": 1e-4} (the
        tracker's reg/shape, reg/exp, reg/jaw), prior={"shape": mica_shape} and init take shape / expression / global_pose / neck /
        jaw / eyes / transl.  A frozen part starts, and stays, at its prior (zero without one) unless init names it.  Returns
        fit's dict and the six FLAME parts [F,n] of the result."""
        who = "MorphableModel.fit_flame"
        if self.J != len(FLAME_JOINTS):
            raise ValueError(f"{who}: a FLAME model has {len(FLAME_JOINTS)} joints, this one {self.J}")
        out = self.fit(target_vertices, target_landmarks, free=free, reg=reg, prior=prior, init=init, _who=who, **kw)
        flat = torch.cat([out["betas"], out["pose"].reshape(out["betas"].shape[0], -1)], 1)
        g = self.param_groups()
        out.update({k: flat[:, g[k]].contiguous() for k in ("shape", "expression", "global_pose", "neck", "jaw", "eyes")})
        return out

    # ---- fitting to an unregistered scan: correspondences by closest point (engine.morph_fit_scan_run, csrc/k_closest.hip)
    def _scan_list(self, who, scan_vertices, scan_faces):
        """[(verts float32 [n,3], faces int32 [k,3])] host tensors: one scan or a list of them; faces None = a point cloud (i, i, i)."""
        many = isinstance(scan_vertices, (list, tuple))
        vs = list(scan_vertices) if many else [scan_vertices]
        if scan_faces is None:
            fs = [None] * len(vs)
        elif many:
            fs = list(scan_faces) if isinstance(scan_faces, (list, tuple)) else None
            if fs is None or len(fs) != len(vs):
                raise ValueError(f"{who}: a list of scans needs a list of as many scan_faces (entries may be None)")
        else:
            fs = [scan_faces]
        if not vs:
            raise ValueError(f"{who}: no scan given")
        out = []
        for i, (sv, sf) in enumerate(zip(vs, fs)):
            sv = (sv.detach().cpu() if torch.is_tensor(sv) else torch.as_tensor(np.asarray(sv))).to(torch.float32)
            if sv.dim() != 2 or sv.shape[1] != 3 or sv.shape[0] < 1:
                raise ValueError(f"{who}: scan {i}: vertices must be [n,3] with n >= 1, got {tuple(sv.shape)}")
            if sf is None:
                sf = torch.arange(sv.shape[0], dtype=torch.int32)[:, None].expand(-1, 3)
            else:
                sf = sf.detach().cpu() if torch.is_tensor(sf) else torch.as_tensor(np.asarray(sf))
                if sf.dim() != 2 or sf.shape[1] != 3 or sf.shape[0] < 1 or sf.is_floating_point():
                    raise ValueError(f"{who}: scan {i}: faces must be integers [k,3] with k >= 1, got {sf.dtype} {tuple(sf.shape)}")
                sf = sf.to(torch.int32)
            out.append((sv.contiguous(), sf.contiguous()))
        return out

    def scan_distance(self, vertices, scans, normal_cos=None, max_dist=None, incidence=None):
        """The closest point of the scan(s) for vertices [F,V,3] of this model (scan f for frame f, or the one scan for all), with
        the gates of fit_scan: dict of face [F,V] int32 (-1: no match), point [F,V,3], dist2 [F,V], matched [F] (a count) and rms
        [F]: the root mean square distance over the matched vertices (NaN where none matched)."""
        F = vertices.shape[0]
        dev = vertices.device
        nrm = None
        if normal_cos is not None:
            nrm, _ = E.op_mesh_vertex_normals(vertices, self.faces, incidence[0], incidence[1], device=dev)
        max_dist2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
        kw = dict(cos_min=0.0 if normal_cos is None else float(normal_cos), max_dist2=max_dist2, device=dev)
        if len(scans) == 1:
            o = E.op_mesh_closest_point(vertices.reshape(-1, 3), scans[0][0], scans[0][1],
                                        query_normals=None if nrm is None else nrm.reshape(-1, 3), **kw)
            outs = {k: o[k].reshape((F, self.V) + tuple(o[k].shape[1:])) for k in ("face", "point", "dist2")}
        else:
            per = [E.op_mesh_closest_point(vertices[f], scans[f][0], scans[f][1], query_normals=None if nrm is None else nrm[f], **kw)
                   for f in range(F)]
            outs = {k: torch.stack([o[k] for o in per]) for k in ("face", "point", "dist2")}
        hit = outs["face"] >= 0
        outs["matched"] = hit.sum(1).to(torch.int32)
        total = torch.where(hit, outs["dist2"], torch.zeros_like(outs["dist2"])).double().sum(1)
        outs["rms"] = (total / outs["matched"].double()).sqrt().float()  # 0 / 0 = NaN: nothing matched
        return outs

    def fit_scan(self, scan_vertices, scan_faces=None, target_landmarks=None, max_dist=None, normal_cos=None, refresh=1, vertex_weight=None,
                 iters=300, lr=0.05, init=None, free=None, reg=None, prior=None, post=None, landmark_weight=None, lmk_lambda=1.0,
                 fit_transl=True, frames=None, _who="MorphableModel.fit_scan"):
        """``fit`` against a scan of ANY topology (raw scans, registrations in another topology, point clouds): every ``refresh``
        iterations each model vertex takes the closest point of the scan as its target (an exhaustive, exact query on the device:
        mesh.closest_point), optionally only among faces whose normal makes a cosine >= normal_cos with the vertex normal and
        within max_dist; unmatched vertices drop out of the data term, E_f = sum_v w_v m_fv |y - c|^2 / sum_v w_v m_fv + the
        landmark and penalty terms of ``fit``.  scan_vertices [n,3] with scan_faces [k,3] (None: a point cloud), or lists of them,
        one scan per frame; ``frames``: how many frames share one scan (default: those of target_landmarks or init, else 1).
        Returns fit's dict plus matched_history [iters,F] and, from a fresh query of the returned vertices with the same gates,
        corr_face [F,V] (-1: no match), matched [F] and rms [F]: the root mean square model-to-scan surface distance over the
        matched vertices.  The start matters as in any ICP: give init (or target_landmarks, whose term stays on) when the scan
        is far from the model's rest pose."""
        who = _who
        lrv, lam, p0 = self.fit_vectors(lr, free, reg, prior, fit_transl, who)
        scans = self._scan_list(who, scan_vertices, scan_faces)
        tl = None if target_landmarks is None else (target_landmarks if torch.is_tensor(target_landmarks)
                                                    else torch.as_tensor(np.asarray(target_landmarks)))
        tl = tl[None] if tl is not None and tl.dim() == 2 else tl
        if tl is not None:
            if self.lmk_face is None:
                raise ValueError(f"{who}: target_landmarks given, and the model has no landmark embedding")
            M = self.lmk_face.shape[0]
            if tl.dim() != 3 or tuple(tl.shape[1:]) != (M, 3) or tl.shape[0] < 1:
                raise ValueError(f"{who}: target_landmarks must be [F,{M},3], got {tuple(tl.shape)}")
        counts = [len(scans), 1 if tl is None else tl.shape[0], 1 if frames is None else int(frames)]
        counts += [int(np.shape(val)[0]) for val in (init or {}).values() if val is not None and np.ndim(val) >= 2]
        F = max(counts)
        if F < 1 or any(c not in (1, F) for c in counts):
            raise ValueError(f"{who}: scans, target_landmarks, init and frames must agree on the number of frames (or be one), got {counts}")
        iters, refresh = int(iters), int(refresh)
        if iters < 1 or refresh < 1:
            raise ValueError(f"{who}: iters and refresh must be at least 1, got {iters} and {refresh}")
        if max_dist is not None and not float(max_dist) > 0.0:
            raise ValueError(f"{who}: max_dist must be positive, got {max_dist}")
        if normal_cos is not None:
            if not -1.0 <= float(normal_cos) <= 1.0:
                raise ValueError(f"{who}: normal_cos must be in [-1, 1], got {normal_cos}")
            if self.faces is None:
                raise ValueError(f"{who}: normal_cos needs the model's faces (vertex normals)")
        start = self._fit_init(who, init, F, p0, lrv)
        if self.device.type != "cuda":
            raise ValueError(f"{who}: the model is on {self.device}; the fitter runs on the GPU only (model.to('cuda:0'))")
        dev = self.device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        incidence = None
        if normal_cos is not None:
            from .mesh import face_incidence
            incidence = tuple(torch.from_numpy(a).to(dev) for a in face_incidence(self.faces, self.V))
        scans = [(a.to(dev), b.to(dev)) for a, b in scans]
        p = f32(start)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        max_dist2 = float("inf") if max_dist is None else float(np.float32(float(max_dist) ** 2))
        hist, matched_hist, _ = E.morph_fit_scan_run(self, p, m, v, f32(lrv), f32(lam), f32(p0), iters, scans, incidence=incidence,
                                                     normal_cos=normal_cos, max_dist2=max_dist2, refresh=refresh,
                                                     vertex_weight=vertex_weight, target_lmk=tl, lmk_weight=landmark_weight,
                                                     lmk_lambda=lmk_lambda, post=post)
        NB, J = self.NB, self.J
        out = {"betas": p[:, :NB].contiguous(), "pose": p[:, NB:NB + 3 * J].reshape(F, J, 3).contiguous(),
               "transl": p[:, NB + 3 * J:].contiguous(), "loss_history": hist, "matched_history": matched_hist}
        out["vertices"] = self.forward(out["betas"], out["pose"], post=post, transl=out["transl"])["vertices"]
        fresh = self.scan_distance(out["vertices"], scans, normal_cos, max_dist, incidence)
        out.update(corr_face=fresh["face"], matched=fresh["matched"], rms=fresh["rms"])
        return out

    def fit_flame_scan(self, scan_vertices, scan_faces=None, target_landmarks=None, free=None, reg=None, prior=None, init=None, **kw):
        """``fit_scan`` in ``flame``'s names, as fit_flame is to fit.  Returns fit_scan's dict and the six FLAME parts [F,n]."""
        who = "MorphableModel.fit_flame_scan"
        if self.J != len(FLAME_JOINTS):
            raise ValueError(f"{who}: a FLAME model has {len(FLAME_JOINTS)} joints, this one {self.J}")
        out = self.fit_scan(scan_vertices, scan_faces, target_landmarks, free=free, reg=reg, prior=prior, init=init, _who=who, **kw)
        flat = torch.cat([out["betas"], out["pose"].reshape(out["betas"].shape[0], -1)], 1)
        g = self.param_groups()
        out.update({k: flat[:, g[k]].contiguous() for k in ("shape", "expression", "global_pose", "neck", "jaw", "eyes")})
        return out

    # ---- fitting to 2-D key points in calibrated views (engine.morph_fit_2d_run, csrc/k_morph_2d.hip)
    def project_landmarks(self, betas, pose, K, RT, transl=None, post=None, z_near=E.Z_NEAR_2D):
        """The forward alone: the model's landmarks in C calibrated views.  K [C,3,3] / RT [C,3,4] (world -> camera; x right, y
        down, z forward; pixel (i, j) centred at (u, v) = (j, i): mesh.project's convention) or [F,C,...] per frame.  Returns device
        tensors: landmarks [F,M,3], uv [F,C,M,2] in pixels, valid [F,C,M] (in front of the camera, finite) and, with a contour
        embedding, rows [F,C] (the row of the contour table each view selects from the head's yaw in it), yaw_deg [F,C],
        contour_landmarks [F,C,Md,3], contour_uv [F,C,Md,2], contour_valid [F,C,Md]."""
        who = "MorphableModel.project_landmarks"
        if self.lmk_face is None:
            raise ValueError(f"{who}: the model has no landmark embedding")
        betas, pose, transl = self._params(who, betas, pose, transl)
        K, RT = (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)) for t in (K, RT))
        r = self._run(betas, pose, post, transl, False)
        uv, valid = E.op_morph_project(r["landmarks"], K, RT, z_near, device=self.device)
        out = {"landmarks": r["landmarks"], "uv": uv, "valid": valid != 0}
        if self.dyn_lmk_face is not None:
            F, C = uv.shape[:2]
            R, Md = self.dyn_lmk_face.shape
            out["rows"], out["yaw_deg"] = E.op_morph_contour_select(r["A"], RT.to(self.device), self.neck_joint, R, device=self.device)
            dyn = E.op_morph_contour_landmarks(r["vertices"], self.faces, self.dyn_lmk_face, self.dyn_lmk_bary, out["rows"], device=self.device)
            # every view's points through every camera, then view c's own block
            uv_all, ok_all = E.op_morph_project(dyn.reshape(F, C * Md, 3), K, RT, z_near, device=self.device)
            pick = torch.arange(C, device=self.device)
            out["contour_landmarks"] = dyn
            out["contour_uv"] = uv_all.reshape(F, C, C, Md, 2)[:, pick, pick]
            out["contour_valid"] = ok_all.reshape(F, C, C, Md)[:, pick, pick] != 0
        return out

    def fit_2d(self, landmarks_2d, K, RT, weights=None, image_size=None, contour_2d=None, contour_weights=None, target_vertices=None,
               vertex_weight=None, lmk2d_lambda=1.0, z_near=E.Z_NEAR_2D, iters=300, lr=0.05, init=None, free=None, reg=None, prior=None,
               post=None, fit_transl=True, landmark_order=None, frames=None, _who="MorphableModel.fit_2d"):
        """Adam on the device against 2-D key points in C calibrated views (the tracker's landmark reprojection term):
        landmarks_2d [C,M,2] or [F,C,M,2] in pixels, K / RT as project_landmarks takes them, weights [C,M] or [F,C,M] (0 = not
        detected; such a target may hold anything, NaN included).  Per frame E_f = lmk2d_lambda sum w |s (uv - target)|^2 / sum w
        over the observations that count (w > 0, at least z_near in front of the camera, finite) + the vertex term of ``fit`` when
        target_vertices is given + sum_p lam_p (p - p0_p)^2; s = 1 / max(H, W) of image_size = (H, W), the tracker's
        normalisation, or 1 without one.  contour_2d [C,Md,2] or [F,C,Md,2] with contour_weights: the face contour, whose model
        points slide with the head's yaw per view (the model needs dyn_lmk_face / dyn_lmk_bary); both sets share one sum of
        weights.  landmark_order="ibug68": landmarks_2d (and weights) hold the 68 iBUG points, of which the first 17 (the jaw
        line) go to the contour set and the other 51 to the static one; the model must have 51 static and 17 contour landmarks.
        A single view with free shape and translation is scale-ambiguous: freeze or regularise the shape, or use two views.
        Returns fit's dict (rms: the root mean square of reprojection_px's distances) plus uv [F,C,M,2], n_valid [F],
        n_valid_history [iters,F], reprojection_px [F,C] (the mean pixel distance of the counted observations of a view, NaN where
        none counts) and, with contours, rows [F,C] and contour_uv [F,C,Md,2]."""
        who = _who
        lrv, lam, p0 = self.fit_vectors(lr, free, reg, prior, fit_transl, who)
        if self.lmk_face is None:
            raise ValueError(f"{who}: the model has no landmark embedding")
        M = self.lmk_face.shape[0]
        ten = lambda t: None if t is None else (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)))
        lm2, w2, ct2, cw2, tv = ten(landmarks_2d), ten(weights), ten(contour_2d), ten(contour_weights), ten(target_vertices)
        if lm2 is None or lm2.dim() not in (3, 4) or lm2.shape[-1] != 2:
            raise ValueError(f"{who}: landmarks_2d must be [C,M,2] or [F,C,M,2], got {None if lm2 is None else tuple(lm2.shape)}")
        if landmark_order == "ibug68":
            if ct2 is not None or cw2 is not None:
                raise ValueError(f"{who}: landmark_order='ibug68' takes the contour from landmarks_2d; do not pass contour_2d as well")
            if self.dyn_lmk_face is None or self.dyn_lmk_face.shape[1] != 17 or M != 51 or lm2.shape[-2] != 68:
                raise ValueError(f"{who}: landmark_order='ibug68' needs 68 points and a model with 51 static and 17 contour landmarks")
            ct2, lm2 = lm2[..., :17, :], lm2[..., 17:, :]
            if w2 is not None:
                cw2, w2 = w2[..., :17], w2[..., 17:]
        elif landmark_order is not None:
            raise ValueError(f"{who}: landmark_order must be None or 'ibug68', got {landmark_order!r}")
        lm2 = lm2[None] if lm2.dim() == 3 else lm2
        C = lm2.shape[1]
        if lm2.shape[2] != M:
            raise ValueError(f"{who}: landmarks_2d has {lm2.shape[2]} points a view, the model {M} static landmarks")
        Md = 0
        if ct2 is not None:
            if self.dyn_lmk_face is None:
                raise ValueError(f"{who}: contour_2d given, and the model has no contour embedding")
            Md = self.dyn_lmk_face.shape[1]
            ct2 = ct2[None] if ct2.dim() == 3 else ct2
            if ct2.dim() != 4 or tuple(ct2.shape[1:]) != (C, Md, 2):
                raise ValueError(f"{who}: contour_2d must be [C,{Md},2] or [F,C,{Md},2] with C = {C}, got {tuple(ct2.shape)}")
        elif cw2 is not None:
            raise ValueError(f"{who}: contour_weights without contour_2d")
        w2 = w2[None] if w2 is not None and w2.dim() == 2 else w2
        cw2 = cw2[None] if cw2 is not None and cw2.dim() == 2 else cw2
        for name, t, n in (("weights", w2, M), ("contour_weights", cw2, Md)):
            if t is not None and (t.dim() != 3 or tuple(t.shape[1:]) != (C, n)):
                raise ValueError(f"{who}: {name} must be [C,{n}] or [F,C,{n}] with C = {C}, got {tuple(t.shape)}")
        tv = tv[None] if tv is not None and tv.dim() == 2 else tv
        if tv is not None and (tv.dim() != 3 or tuple(tv.shape[1:]) != (self.V, 3)):
            raise ValueError(f"{who}: target_vertices must be [F,{self.V},3] (the model's topology), got {tuple(tv.shape)}")
        Kt, RTt = ten(K), ten(RT)
        counts = [t.shape[0] for t in (lm2, w2, ct2, cw2, tv) if t is not None] + [1 if frames is None else int(frames)]
        counts += [t.shape[0] for t in (Kt, RTt) if t.dim() == 4]
        counts += [int(np.shape(val)[0]) for val in (init or {}).values() if val is not None and np.ndim(val) >= 2]
        F = max(counts)
        if F < 1 or any(c not in (1, F) for c in counts):
            raise ValueError(f"{who}: the targets, weights, cameras, init and frames must agree on the number of frames (or be one), got {counts}")
        grow = lambda t: None if t is None else (t if t.shape[0] == Ft else t.expand((Ft,) + tuple(t.shape[1:])))
        Ft = max(t.shape[0] for t in (lm2, w2, ct2, cw2) if t is not None)
        lm2, w2, ct2, cw2 = grow(lm2), grow(w2), grow(ct2), grow(cw2)
        px_scale = 1.0
        if image_size is not None:
            hw = [float(x) for x in np.asarray(image_size).reshape(-1)]
            if len(hw) not in (1, 2) or not all(0.0 < x < float("inf") for x in hw):
                raise ValueError(f"{who}: image_size must be (H, W) or one positive number, got {image_size}")
            px_scale = 1.0 / max(hw)
        iters = int(iters)
        if iters < 1:
            raise ValueError(f"{who}: iters must be at least 1, got {iters}")
        start = self._fit_init(who, init, F, p0, lrv)
        if self.device.type != "cuda":
            raise ValueError(f"{who}: the model is on {self.device}; the fitter runs on the GPU only (model.to('cuda:0'))")
        dev = self.device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        p = f32(start)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        hist, n_hist = E.morph_fit_2d_run(self, p, m, v, f32(lrv), f32(lam), f32(p0), iters, Kt, RTt, lm2, weight=w2, dyn_target_uv=ct2,
                                          dyn_weight=cw2, z_near=z_near, px_scale=px_scale, lambda2=lmk2d_lambda, target=tv,
                                          vertex_weight=vertex_weight, post=post)
        NB, J = self.NB, self.J
        out = {"betas": p[:, :NB].contiguous(), "pose": p[:, NB:NB + 3 * J].reshape(F, J, 3).contiguous(),
               "transl": p[:, NB + 3 * J:].contiguous(), "loss_history": hist, "n_valid_history": n_hist}
        fw = self.forward(out["betas"], out["pose"], post=post, transl=out["transl"])
        out["vertices"] = fw["vertices"]
        pr = self.project_landmarks(out["betas"], out["pose"], Kt, RTt, transl=out["transl"], post=post, z_near=z_near)
        out["uv"] = pr["uv"]
        got, want, ok, wt = [pr["uv"]], [lm2], [pr["valid"]], [w2]
        if ct2 is not None:
            out["rows"], out["contour_uv"] = pr["rows"], pr["contour_uv"]
            got, want, ok, wt = got + [pr["contour_uv"]], want + [ct2], ok + [pr["contour_valid"]], wt + [cw2]
        dist, counted = [], []
        for g_, t_, o_, w_ in zip(got, want, ok, wt):
            t_ = t_.to(device=dev, dtype=torch.float32)
            c_ = o_ if w_ is None else o_ & (w_.to(dev) > 0)
            d_ = (g_ - t_).square().sum(-1).sqrt()
            dist.append(torch.where(c_, d_, torch.zeros_like(d_)))  # an uncounted target may be NaN
            counted.append(c_.expand_as(d_))
        dist, counted = torch.cat(dist, -1), torch.cat(counted, -1)
        n = counted.sum(-1)
        out["n_valid"] = n.sum(-1).to(torch.int32)
        out["reprojection_px"] = dist.sum(-1) / n  # 0 / 0 = NaN: nothing counts in that view
        out["rms"] = (dist.square().sum((-1, -2)) / n.sum(-1)).sqrt()
        return out

    def fit_flame_2d(self, landmarks_2d, K, RT, free=None, reg=None, prior=None, init=None, **kw):
        """``fit_2d`` in ``flame``'s names, as fit_flame is to fit.  Returns fit_2d's dict and the six FLAME parts [F,n]."""
        who = "MorphableModel.fit_flame_2d"
        if self.J != len(FLAME_JOINTS):
            raise ValueError(f"{who}: a FLAME model has {len(FLAME_JOINTS)} joints, this one {self.J}")
        out = self.fit_2d(landmarks_2d, K, RT, free=free, reg=reg, prior=prior, init=init, _who=who, **kw)
        flat = torch.cat([out["betas"], out["pose"].reshape(out["betas"].shape[0], -1)], 1)
        g = self.param_groups()
        out.update({k: flat[:, g[k]].contiguous() for k in ("shape", "expression", "global_pose", "neck", "jaw", "eyes")})
        return out

    def flame(self, shape, expression=None, global_pose=None, neck=None, jaw=None, eyes=None, post=None, transl=None):
        """The reference's FLAME.forward (flame.py:252-279): betas = [shape, expression], full_pose = [global, neck, jaw, eyes]
        (3, 3, 3 and 6 numbers); missing parts are zero.  Every argument is a vector or has a leading frame axis; single rows
        are repeated for every frame.  transl [3] or [F,3]: see forward."""
        if self.J != len(FLAME_JOINTS):
            raise ValueError(f"MorphableModel.flame: a FLAME model has {len(FLAME_JOINTS)} joints, this one {self.J}")
        parts = {"shape": shape, "expression": expression, "global_pose": global_pose, "neck": neck, "jaw": jaw, "eyes": eyes}
        F = max([1] + [int(v.shape[0]) for v in parts.values() if v is not None and np.ndim(v) == 2])
        sh = np.asarray(shape.detach().cpu() if torch.is_tensor(shape) else shape)
        n_sh = sh.shape[-1]
        if n_sh > self.NB:
            raise ValueError(f"MorphableModel.flame: shape has {n_sh} entries, the model {self.NB} betas")
        betas = np.concatenate([_rows(shape, F, n_sh, "shape"), _rows(expression, F, self.NB - n_sh, "expression")], 1)
        pose = np.concatenate([_rows(global_pose, F, 3, "global_pose"), _rows(neck, F, 3, "neck"), _rows(jaw, F, 3, "jaw"),
                               _rows(eyes, F, 6, "eyes")], 1)
        transl = None if transl is None else torch.from_numpy(np.array(_rows(transl, F, 3, "transl")))
        return self.forward(torch.from_numpy(betas), torch.from_numpy(pose), post=post, transl=transl)

    def to(self, device):
        self.device = torch.device(device)
        for k in ("v_template", "basis", "weights", "j_template", "j_dirs", "faces", "lmk_face", "lmk_bary", "csr_ptr", "csr_ent",
                  "dyn_lmk_face", "dyn_lmk_bary", "ct_vert", "ct_ptr", "ct_ent"):
            if getattr(self, k) is not None:
                setattr(self, k, getattr(self, k).to(self.device))
        return self


class _MorphFunction(torch.autograd.Function):
    """MorphableModel.differentiable: the forward's launches, and in backward those of MorphableModel.vjp."""

    @staticmethod
    def forward(ctx, model, post, has_transl, betas, pose, transl):
        b, p, t = model._params("MorphableModel.differentiable", betas, pose, transl if has_transl else None)
        r = model._run(b, p, post, t, True)
        ctx.model, ctx.post, ctx.saved, ctx.pose_shape = model, post, r, pose.shape
        ctx.dtypes = (betas.dtype, pose.dtype, transl.dtype)
        lmk = r["landmarks"] if r["landmarks"] is not None else r["vertices"].new_zeros(())
        ctx.set_materialize_grads(False)  # an output nobody used arrives as None, as in vjp
        ctx.mark_non_differentiable(*([lmk] if r["landmarks"] is None else []))
        return r["vertices"], r["joints"], lmk

    @staticmethod
    def backward(ctx, g_verts, g_joints, g_lmk):
        model = ctx.model
        g = model._backward(ctx.saved, ctx.post, g_verts, g_joints, g_lmk if model.lmk_face is not None else None)
        gb, gp, gt = (x.to(d) for x, d in zip((g["betas"], g["pose"].reshape(ctx.pose_shape), g["transl"]), ctx.dtypes))
        return None, None, None, gb, gp, gt


class _ProjectFunction(torch.autograd.Function):
    """project: mvd_op_morph_project, and in backward mvd_op_morph_project_bwd."""

    @staticmethod
    def forward(ctx, points, K, RT, z_near):
        uv, valid = E.op_morph_project(points, K, RT, z_near)
        ctx.save_for_backward(points, K, RT)
        ctx.z_near = z_near
        ctx.mark_non_differentiable(valid)
        return uv, valid

    @staticmethod
    def backward(ctx, g_uv, _g_valid):
        points, K, RT = ctx.saved_tensors
        g = E.op_morph_project_bwd(points, K, RT, g_uv.contiguous(), ctx.z_near)
        return g.to(points.dtype), None, None, None


def project(points, K, RT, z_near=E.Z_NEAR_2D):
    """points [F,M,3] (the landmarks, joints or vertices of ``MorphableModel.differentiable``, on the GPU) in C calibrated views, K
    [C,3,3] / RT [C,3,4] or [F,C,...]: (uv [F,C,M,2] in pixels, valid [F,C,M] bool).  uv carries gradients to the points through
    the library's own backward, so a 2-D objective of one's own can be written in torch; a view in which a point is not valid
    (behind z_near, not finite) passes no gradient to it.  The cameras are constants."""
    if not torch.is_tensor(points) or not points.is_cuda:
        raise ValueError("project: points must be a tensor on the GPU")
    K, RT = (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)) for t in (K, RT))
    uv, valid = _ProjectFunction.apply(points, K.detach().to(points.device), RT.detach().to(points.device), float(z_near))
    return uv, valid != 0


def reprojection_error(uv, target, weights=None, valid=None, thresholds=(2.0, 4.0, 8.0)):
    """The read-out of a 2-D fit: uv and target [...,C,M,2] in pixels (tensors or arrays), weights [...,C,M] (0 = not detected) and
    valid [...,C,M] (project's) or None.  Over the observations with weight > 0 that are valid, with a finite prediction and
    target: {"mean_px" [...,C]: the mean pixel distance of a view (NaN where nothing counts), "pck" {threshold: [...,C]}: the
    share of its points within that many pixels, "count" [...,C]}; float64 numpy."""
    a = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    u, t = a(uv).astype(np.float64), a(target).astype(np.float64)
    if u.shape != t.shape or u.ndim < 3 or u.shape[-1] != 2:
        raise ValueError(f"reprojection_error: uv and target must both be [...,C,M,2], got {u.shape} and {t.shape}")
    ok = np.isfinite(u).all(-1) & np.isfinite(t).all(-1)
    for name, x in (("weights", weights), ("valid", valid)):
        if x is not None:
            x = a(x)
            if x.shape != u.shape[:-1]:
                raise ValueError(f"reprojection_error: {name} must be {list(u.shape[:-1])}, got {x.shape}")
            ok &= x > 0
    d = np.where(ok, np.sqrt(((np.where(ok[..., None], u - t, 0.0)) ** 2).sum(-1)), 0.0)
    n = ok.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"mean_px": d.sum(-1) / n, "count": n, "pck": {}}
        for thr in thresholds:
            out["pck"][float(thr)] = (ok & (d <= float(thr))).sum(-1) / n
    return out


def flame_alignment() -> torch.Tensor:
    """batch.align_flame_vertices as one 3x4 (float64): x -> S (2.5 (R (1.087 x) + T)) with S the axis swap, composed in
    float64; pass it as ``post`` and the similarity rides along in the skinning pass."""
    pose = torch.tensor(B.FLAME_POSE, dtype=torch.float64)
    R = B.so3_exponential_map(pose[None, :3])[0]
    S = torch.tensor([[1., 0., 0.], [0., 0., 1.], [0., -1., 0.]], dtype=torch.float64)
    return torch.cat([S @ R * (2.5 * B.FLAME_SCALE), (S @ pose[3:] * 2.5)[:, None]], 1)


def interpolate_params(a, b, K):
    """K frames from parameter set ``a`` to ``b`` (dicts of vectors, e.g. shape / expression / jaw): every key of either, a
    key missing on one side being zero there; betas linearly, poses linearly in axis-angle.  Frame 0 is ``a`` and frame K - 1
    is ``b`` exactly (K = 1: ``b``).  Returns {key: float64 array [K,n]}."""
    K = int(K)
    if K < 1:
        raise ValueError(f"interpolate_params: K must be at least 1, got {K}")
    t = np.linspace(0.0, 1.0, K)[:, None] if K > 1 else np.ones((1, 1))
    out = {}
    for k in list(a) + [k for k in b if k not in a]:
        x, y = (None if d.get(k) is None else np.asarray(d[k], dtype=np.float64).reshape(-1) for d in (a, b))
        x = np.zeros_like(y) if x is None else x
        y = np.zeros_like(x) if y is None else y
        if x.shape != y.shape:
            raise ValueError(f"interpolate_params: {k} has {x.shape[0]} entries on one side and {y.shape[0]} on the other")
        out[k] = (1.0 - t) * x[None] + t * y[None]  # t = 0 and t = 1 give the end points exactly
    return out


def frames_to_batch(input_image, vertices_F, num_views=16, image_size=256, device="cpu", cameras=None):
    """batch.build_batch for every frame of vertices_F [F,Nv,3] (already in the cube frame: post=flame_alignment()) with the
    same input image and cameras, stacked by batch.stack_batches: a batch of F samples for model.sample."""
    if vertices_F.dim() != 3 or vertices_F.shape[2] != 3 or vertices_F.shape[0] < 1:
        raise ValueError(f"frames_to_batch: vertices must be [F,Nv,3], got {tuple(vertices_F.shape)}")
    return B.stack_batches([B.build_batch(input_image, v, num_views=num_views, image_size=image_size, device=device, cameras=cameras)
                            for v in vertices_F])
