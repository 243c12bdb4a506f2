"""Dense field extraction (reference: grid_opt/utils/utils_sdf.py:69-86).  The reference
evaluates res^3 queries in 16^3-point chunks -- 4 096 model calls and as many ``.cpu()`` syncs
at resolution 256.  Here the lattice is generated on the device slab by slab (a few million
points per call, forward-only fused encode+decode) and copied to the host once.

Mesh extraction (reference :89-140) runs on the volume where it lies: ``extract_geometry`` hands the
device-resident volume to the HIP marching cubes (``ops.marching_cubes``; the reference copies it to the
host for PyMCubes) and ``save_mesh`` writes the PLY itself -- mcubes, trimesh and open3d are not needed;
the returned ``TriangleMesh`` carries the arrays an open3d mesh would (vertices, triangles, vertex_normals).

Sphere tracing (reference :197-236) is the reference's loop over any callable, and ONE launch when the callable is a
GridAtlas / GridNet queried without autograd on the device (``model.sphere_trace``); ``render_depth`` turns it into
the depth and normal image of a camera pose -- the cheap view of a map now that the Open3D viewers are stubs."""
import logging
import os

import numpy as np
import torch

import miso_amd.grid_opt.utils.utils as utils   # noqa: F401  (the demos reach `utils` through `from ...utils_sdf import *`)

logger = logging.getLogger(__name__)


def sign_mask_from_gt_sdf(gt_sdf: torch.Tensor, trunc_dist=0.15) -> torch.Tensor:
    """(N,1) labels: 1 where sdf > trunc_dist (free space), else 0 (reference :19-37), without the host syncs."""
    return (gt_sdf > trunc_dist).to(gt_sdf.dtype)


def valid_mask_from_gt_sdf(gt_sdf: torch.Tensor, trunc_dist=0.15) -> torch.Tensor:
    """(N,1) labels: 1 where |sdf| < trunc_dist (reference :40-58)."""
    return (gt_sdf.abs() < trunc_dist).to(gt_sdf.dtype)


def extract_fields(bound_min: torch.Tensor, bound_max: torch.Tensor, resolution, query_func,
                   device=None, max_points=1 << 22):
    """u[i,j,k] = query_func((x_i, y_j, z_k)) on the res^3 lattice spanned by linspace per axis,
    returned as a float32 numpy array of shape (res, res, res) like the reference."""
    return extract_fields_device(bound_min, bound_max, resolution, query_func, device, max_points).cpu().numpy()


def extract_fields_device(bound_min: torch.Tensor, bound_max: torch.Tensor, resolution, query_func,
                          device=None, max_points=1 << 22, lattice_func=None) -> torch.Tensor:
    """extract_fields with the (res, res, res) volume left on the device (what marching cubes reads).
    lattice_func(xs, ys, zs) -> (nx, ny, nz) volume or None: a model that evaluates a meshgrid lattice itself (GridAtlas.
    sdf_on_lattice: one launch per slab, the points generated inside the kernel from the three axis vectors); tried
    first, slabs of at most 2^30 points."""
    lo = bound_min.detach().cpu()
    hi = bound_max.detach().cpu()
    if device is None:
        device = "cuda:0" if torch.cuda.is_available() else "cpu"
    axes = [torch.linspace(float(lo[a]), float(hi[a]), resolution) for a in range(3)]   # host linspace, as upstream
    if lattice_func is not None:
        out = torch.empty((resolution, resolution, resolution), dtype=torch.float32, device=device)
        ys_d, zs_d = axes[1].to(device), axes[2].to(device)
        slab = max(1, (1 << 30) // (resolution * resolution))
        ok = True
        for x0 in range(0, resolution, slab):
            vol = lattice_func(axes[0][x0:x0 + slab].to(device), ys_d, zs_d)
            if vol is None:
                ok = False
                break
            out[x0:x0 + vol.shape[0]] = vol
        if ok:
            return out
    ys, zs = axes[1].to(device), axes[2].to(device)
    out = torch.empty((resolution, resolution, resolution), dtype=torch.float32, device=device)
    slab = max(1, max_points // (resolution * resolution))
    with torch.no_grad():
        for x0 in range(0, resolution, slab):
            xs = axes[0][x0:x0 + slab].to(device)
            xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
            pts = torch.stack((xx, yy, zz), dim=-1).reshape(-1, 3)
            out[x0:x0 + xs.shape[0]] = query_func(pts).reshape(xs.shape[0], resolution, resolution)
    return out


def extract_geometry(bound_min: torch.Tensor, bound_max: torch.Tensor, resolution, threshold, query_func,
                     device=None, lattice_func=None):
    """Level set ``threshold`` of the field as (vertices (V,3) float64 in metres, triangles (T,3) int64), numpy
    (reference :89-101).  Vertices in index coordinates are mapped to the bound exactly as upstream:
    ``v / (res - 1) * (max - min) + min``."""
    from miso_amd import ops
    u = extract_fields_device(bound_min, bound_max, resolution, query_func, device, lattice_func=lattice_func)
    verts, tris = ops.marching_cubes(u, float(threshold))
    lo = bound_min.detach().cpu().numpy()
    hi = bound_max.detach().cpu().numpy()
    vertices = verts.cpu().numpy().astype(np.float64) / (resolution - 1.0) * (hi - lo)[None, :] + lo[None, :]
    return vertices, tris.cpu().numpy()


class TriangleMesh:
    """The arrays of the open3d mesh the reference's save_mesh returns."""

    def __init__(self, vertices, triangles):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        self.vertex_normals = None

    def apply_transform(self, T):
        T = np.asarray(T, dtype=np.float64)
        self.vertices = self.vertices @ T[:3, :3].T + T[:3, 3][None, :]
        return self

    def compute_vertex_normals(self):
        """Area-weighted average of the incident face normals, normalised."""
        v, f = self.vertices, self.triangles
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        vn = np.zeros_like(v)
        for k in range(3):
            np.add.at(vn, f[:, k], fn)
        norm = np.linalg.norm(vn, axis=1, keepdims=True)
        self.vertex_normals = vn / np.where(norm > 0, norm, 1.0)
        return self

    def export_ply(self, path):
        """Binary little-endian PLY: float32 x y z per vertex, uchar-counted int32 index lists per face (what
        trimesh's ``export(file_type='ply')`` writes for a bare mesh)."""
        v = self.vertices.astype('<f4')
        f = np.empty(len(self.triangles), dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
        f['n'] = 3
        f['idx'] = self.triangles
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, 'wb') as fh:
            fh.write(header.encode('ascii'))
            fh.write(v.tobytes())
            fh.write(f.tobytes())


def box_mesh(bound) -> TriangleMesh:
    """The six rectangles of the axis-aligned box ``bound`` ((3, 2) rows [min, max]) as twelve triangles."""
    b = np.asarray(bound, dtype=np.float64).reshape(3, 2)
    v = np.array([[x, y, z] for x in b[0] for y in b[1] for z in b[2]])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return TriangleMesh(v, [t for a, c, d, e in quads for t in ((a, c, d), (a, d, e))])


_PLY_SCALARS = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
                'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
                'double': 'f8', 'float64': 'f8'}


def _ply_header(fh):
    """-> (format, [(element name, count, [(property name, scalar dtype) | (name, count dtype, item dtype)])])"""
    if fh.readline().strip() != b'ply':
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        raw = fh.readline()
        if not raw:
            raise ValueError("PLY header without end_header")
        w = raw.decode('ascii', 'replace').split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            if not elements:
                raise ValueError("PLY property before any element")
            types = w[2:4] if w[1] == 'list' else w[1:2]
            if any(t not in _PLY_SCALARS for t in types):
                raise ValueError(f"PLY property of unknown type: {' '.join(w)}")
            elements[-1][2].append((w[-1],) + tuple(_PLY_SCALARS[t] for t in types))
        elif w[0] == 'end_header':
            break
        else:
            raise ValueError(f"cannot read PLY header line '{' '.join(w)}'")
    if fmt not in ('binary_little_endian', 'ascii'):
        raise ValueError(f"PLY format '{fmt}' is not read (binary_little_endian and ascii are)")
    return fmt, elements


def read_ply(path) -> TriangleMesh:
    """A PLY mesh or point cloud -> TriangleMesh (no face element: zero triangles).  Reads ``binary_little_endian`` and
    ``ascii`` files whose vertex element has x, y, z and any further scalar properties of any PLY scalar type (ScanNet's
    colours, normals ...), which are skipped, and whose faces are uchar- or int-counted index lists of three; that
    includes what TriangleMesh.export_ply writes.  ValueError: a face that is not a triangle, another format
    (big-endian), a list property on the vertices, or an element that cannot be skipped (a list in a binary file)."""
    with open(path, 'rb') as fh:
        fmt, elements = _ply_header(fh)
        verts, tris = None, np.zeros((0, 3), dtype=np.int64)
        tokens = fh.read().split() if fmt == 'ascii' else None
        at = 0
        for name, count, props in elements:
            lists = [p for p in props if len(p) == 3]
            if name == 'face' and len(props) >= 1 and len(lists) == 1 and props[0] is lists[0]:
                extra = props[1:]
                if any(len(p) == 3 for p in extra):
                    raise ValueError("PLY face element with more than one list")
                if fmt == 'ascii':
                    width = 4 + len(extra)
                    chunk = tokens[at:at + count * width]
                    if len(chunk) < count * width or any(int(float(v)) != 3 for v in chunk[::width]):
                        raise ValueError("PLY faces must be triangles")
                    if count:
                        tris = np.asarray(chunk, dtype=np.float64).reshape(count, width)[:, 1:4].astype(np.int64)
                    at += count * width
                else:
                    dt = np.dtype([('n', '<' + lists[0][1]), ('idx', '<' + lists[0][2], (3,))] +
                                  [(f'_{i}', '<' + p[1]) for i, p in enumerate(extra)])
                    data = fh.read(dt.itemsize * count)
                    n_ok = len(data) // dt.itemsize
                    f = np.frombuffer(data[:n_ok * dt.itemsize], dtype=dt)
                    if n_ok < count or (count and not (f['n'] == 3).all()):
                        raise ValueError("PLY faces must be triangles")
                    tris = f['idx'].astype(np.int64)
                continue
            if lists:
                if name == 'vertex' or fmt != 'ascii':
                    raise ValueError(f"PLY element '{name}' has a list property and cannot be " +
                                     ("read" if name == 'vertex' else "skipped"))
                for _ in range(count):                       # ascii: every list states its length
                    for p in props:
                        at += 1 + int(float(tokens[at])) if len(p) == 3 else 1
                continue
            if fmt == 'ascii':
                block = np.asarray(tokens[at:at + count * len(props)], dtype=np.float64).reshape(count, len(props))
                at += count * len(props)
                cols = {p[0]: block[:, i] for i, p in enumerate(props)}
            else:
                dt = np.dtype([(p[0], '<' + p[1]) for p in props])
                data = fh.read(dt.itemsize * count)
                if len(data) < dt.itemsize * count:
                    raise ValueError(f"PLY element '{name}' is cut short")
                cols = np.frombuffer(data, dtype=dt)
            if name == 'vertex':
                if any(k not in [p[0] for p in props] for k in 'xyz'):
                    raise ValueError("PLY vertex element without x, y, z")
                verts = np.stack([np.asarray(cols[k], dtype=np.float64) for k in 'xyz'], axis=1)
        if verts is None:
            raise ValueError("PLY file without a vertex element")
    return TriangleMesh(verts, tris)


def save_mesh(model, bounds: torch.Tensor, save_path=None, resolution=256, device='cuda:0', flip_face=True,
              transform: torch.Tensor = None) -> TriangleMesh:
    """Zero level set of ``model`` inside ``bounds`` ((3,2) rows [min,max]) as a triangle mesh, optionally moved by
    the 4x4 ``transform`` and written as PLY (reference :104-140)."""
    if save_path is not None:
        logger.info(f"Saving mesh to {save_path}...")
        os.makedirs(os.path.dirname(save_path), exist_ok=True)

    def query_func(pts):
        with torch.no_grad():
            return model(pts.to(device))

    vertices, triangles = extract_geometry(bounds[:, 0], bounds[:, 1], resolution=resolution, threshold=0,
                                           query_func=query_func, device=device,
                                           lattice_func=getattr(model, 'sdf_on_lattice', None))
    if flip_face:
        triangles = triangles[:, [2, 1, 0]]
    mesh = TriangleMesh(vertices, triangles)
    if transform is not None:
        mesh.apply_transform(transform.detach().cpu().numpy())
    if save_path is not None:
        mesh.export_ply(save_path)
    return mesh.compute_vertex_normals()


def sphere_tracing(query_func, origins, directions, min_dist=1e-3, max_dist=5e1, max_iters=100, epsilon=1e-5):
    """March N rays through the SDF ``query_func`` (reference :197-236).  origins, directions: (N,3).
    -> points (N,3), the ray-surface intersections (arbitrary for rays that do not hit), and mask (N,1) bool, true for
    the rays that hit.  A model (or its bound forward) that has ``sphere_trace`` serves the call in one launch when
    autograd is off and the tensors are on the device; anything else runs the loop below."""
    n = origins.shape[0]
    assert origins.ndim == 2 and directions.ndim == 2, f"Wrong shape: origins {origins.shape}, directions {directions.shape}"
    assert directions.shape[0] == n
    if max_iters < 1:
        raise ValueError(f"max_iters must be at least 1, got {max_iters}")   # (upstream: an unbound name at the return)
    model = getattr(query_func, '__self__', query_func)
    if hasattr(model, 'sphere_trace') and not torch.is_grad_enabled() and origins.is_cuda and directions.is_cuda:
        got = model.sphere_trace(origins, directions, min_dist=min_dist, max_dist=max_dist, max_iters=max_iters,
                                 epsilon=epsilon)
        if got is not None:
            return got[0], got[1].reshape(-1, 1)
    directions = utils.normalize_last_dim(directions)
    points = origins + min_dist * directions
    for i in range(max_iters):
        dists = torch.norm(points - origins, dim=1, keepdim=True)
        sdfs = query_func(points)
        mask_converge = sdfs < epsilon
        mask_far = dists > max_dist
        mask_stop = torch.logical_or(mask_converge, mask_far)
        if torch.sum(mask_stop) == n:       # all rays finished
            break
        points = mask_stop * points + ~mask_stop * (points + sdfs * directions)
    return points, mask_converge.reshape(-1, 1)


def render_depth(model, R_world_cam, t_world_cam, cam, H=None, W=None, max_dist=5e1, normals=False, **trace_kw):
    """Depth image of the field ``model`` seen by the pinhole ``cam`` (utils_data.CameraParameters) at the pose
    (R_world_cam (3,3), t_world_cam (3,) or (3,1)): one sphere-traced ray per pixel (utils_sample.ray_dirs_C, row-major).
    -> (depth (H,W), mask (H,W) bool[, normals (H,W,3)]): z-depth in metres -- the ray parameter over the length of the
    unnormalised direction ((c-cx)/fx, (r-cy)/fy, 1) -- and 0 where the ray did not hit, the "0 = no return" of a
    PosedSdfRgbd frame; with normals=True unit normals in the world frame from central differences of the field at the
    hit points (``grad_step`` in trace_kw, default 1e-2: diff.gradient3d's), zero where not hit.  H, W default to the
    camera's; trace_kw: min_dist, max_iters, epsilon.  The device is the model's."""
    import miso_amd.grid_opt.utils.utils_sample as utils_sample
    from miso_amd.grid_opt import diff
    H = int(cam.H if H is None else H)
    W = int(cam.W if W is None else W)
    grad_step = trace_kw.pop('grad_step', 1e-2)
    p0 = next(model.parameters(), None) if hasattr(model, 'parameters') else None
    device = R_world_cam.device if p0 is None else p0.device
    R = R_world_cam.detach().to(device=device, dtype=torch.float32).reshape(3, 3)
    t = t_world_cam.detach().to(device=device, dtype=torch.float32).reshape(1, 3)
    dirs_c = utils_sample.ray_dirs_C(1, H, W, cam.fx, cam.fy, cam.cx, cam.cy, device, 'z').reshape(-1, 3)
    dirs_w = dirs_c @ R.T
    origins = t.expand(H * W, 3).contiguous()
    grad = None
    with torch.no_grad():
        fused = None
        if hasattr(model, 'sphere_trace') and origins.is_cuda:
            fused = model.sphere_trace(origins, dirs_w, max_dist=max_dist,
                                       grad_step=grad_step if normals else None, **trace_kw)
        if fused is not None:
            points, mask, extras = fused
            grad = extras.get('grad')
        else:
            points, mask = sphere_tracing(lambda p: model(p), origins, dirs_w, max_dist=max_dist, **trace_kw)
            if normals:
                grad = diff.gradient3d(points, model, 'finitediff', grad_step)
        mask = mask.reshape(-1, 1)
        depth = torch.norm(points - origins, dim=1, keepdim=True) / torch.norm(dirs_c, dim=1, keepdim=True)
        depth = torch.where(mask, depth, torch.zeros_like(depth)).reshape(H, W)
        if not normals:
            return depth, mask.reshape(H, W)
        nrm = utils.normalize_last_dim(grad)
        nrm = torch.where(mask, nrm, torch.zeros_like(nrm)).reshape(H, W, 3)
    return depth, mask.reshape(H, W), nrm


def _mesh_arrays(mesh, device):
    """a TriangleMesh or a PLY path -> (vertices (V, 3) fp32, triangles (T, 3) int64) on ``device``"""
    if isinstance(mesh, (str, os.PathLike)):
        mesh = read_ply(mesh)
    return (torch.as_tensor(np.asarray(mesh.vertices), dtype=torch.float32, device=device),
            torch.as_tensor(np.asarray(mesh.triangles), dtype=torch.int64, device=device))


def mesh_cast_rays(mesh, origins, dirs, t_min=0.0, t_max=float('inf')):
    """First hit of every ray on ``mesh`` -- an ops.MeshIndex (the HIP grid walk), or a TriangleMesh / PLY path, which goes
    to ops.cast_rays on a HIP device and to utils_geometry.cast_rays_torch on the CPU.
    -> (t (N,), tri (N,) int64, normals_of (callable: tri -> (N, 3) unit winding normals of the hit triangles))."""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_geometry
    if isinstance(mesh, ops.MeshIndex):
        t, tri = mesh.cast_rays(origins, dirs, t_min, t_max)
        verts, tris = mesh.vertices, mesh.triangles
    else:
        verts, tris = _mesh_arrays(mesh, origins.device)
        if origins.is_cuda:
            t, tri = ops.cast_rays(origins, dirs, verts, tris, t_min, t_max)
        else:
            chunk = max(1, min(4096, (1 << 22) // max(int(tris.shape[0]), 1)))
            t, tri = utils_geometry.cast_rays_torch(origins, dirs, verts, tris, t_min, t_max, chunk=chunk)

    def normals_of(tri_idx):
        if not int(tris.shape[0]) or not int(verts.shape[0]):
            return origins.new_zeros((int(tri_idx.shape[0]), 3))
        v = verts[tris[tri_idx.clamp(min=0)].clamp(0, max(int(verts.shape[0]) - 1, 0))]
        n = torch.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], dim=1)
        return utils.normalize_last_dim(n)

    return t, tri, normals_of


def _mesh_inside_and_distance(mesh, points):
    """-> (distance (N,) >= 0, inside (N,) bool) of ``points`` (N, 3) fp32 against ``mesh``, by the route of their device:
    an ops.MeshIndex or a HIP tensor goes to MeshIndex.closest / contains (csrc/mesh_sdf.hip), a CPU tensor to
    utils_geometry.closest_on_mesh_torch / count_crossings_torch with the same three parity directions."""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_geometry
    if not isinstance(mesh, ops.MeshIndex) and points.is_cuda:
        mesh = ops.MeshIndex(*_mesh_arrays(mesh, points.device))
    if isinstance(mesh, ops.MeshIndex):
        return mesh.closest(points)[0].sqrt(), mesh.contains(points)
    verts, tris = _mesh_arrays(mesh, points.device)
    n = int(points.shape[0])
    chunk = max(1, min(4096, (1 << 21) // max(int(tris.shape[0]), 1)))
    d = utils_geometry.closest_on_mesh_torch(points, verts, tris, chunk=chunk)[0].sqrt()
    dirs = torch.tensor(ops.MESH_PARITY_DIRS, dtype=points.dtype, device=points.device)
    odd = utils_geometry.count_crossings_torch(points.repeat(3, 1), dirs.repeat_interleave(n, dim=0), verts, tris,
                                               chunk=chunk).view(3, n) & 1
    return d, odd.sum(dim=0) >= 2


def mesh_signed_distance(mesh, points, inside_positive=True):
    """Signed distance from ``points`` (N, 3) fp32 to ``mesh`` -- an ops.MeshIndex, or a TriangleMesh / PLY path -- routed
    by the points' device like mesh_cast_rays.  The magnitude is the distance to the closest triangle; the sign comes from
    crossing parity (the vote of ops.MESH_PARITY_DIRS), which means inside only for a closed surface.  -> (N,) fp32,
    positive inside with ``inside_positive`` (pysdf's convention: MeshSdf); +inf where the mesh has no triangle."""
    d, inside = _mesh_inside_and_distance(mesh, points)
    return torch.where((inside == bool(inside_positive)) | ~torch.isfinite(d), d, -d)      # THE sign, here and nowhere else


class MeshSdf:
    """The pysdf-shaped callable the reference builds with ``pysdf.SDF(vertices, faces)``: ``f(points) -> (N,) float32``,
    numpy in, numpy out, and ``f.contains(points) -> (N,) bool``.
    Sign: **positive inside**, negative outside.  pysdf cannot be installed beside this project, so the convention rests
    on its documentation ("SDF is > 0 inside and < 0 outside") and on how the reference uses it: PosedSdf3D accepts a
    camera position where ``sdf_fn(p) > 0.3``, i.e. at least 0.3 m inside the room shell (grid_opt/datasets/sdf_3d.py:193-199).
    The sign is set in one line, mesh_signed_distance's.  ``device``: where the queries run (default: the HIP device when
    there is one, else the CPU); on a HIP device the index is built once and kept."""

    def __init__(self, vertices, faces, device=None):
        self.device = torch.device(device if device is not None else ('cuda:0' if torch.cuda.is_available() else 'cpu'))
        self.mesh = TriangleMesh(vertices, faces)
        if self.device.type == 'cuda':
            from miso_amd import ops
            self.mesh = ops.MeshIndex(*_mesh_arrays(self.mesh, self.device))

    def _points(self, points):
        return torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).to(self.device)

    def on_device(self, points):
        """``points`` (N, 3) fp32 tensor on self.device -> (N,) fp32 tensor there: no host round trip"""
        return mesh_signed_distance(self.mesh, points, inside_positive=True)

    def __call__(self, points):
        return self.on_device(self._points(points)).cpu().numpy().astype(np.float32)

    def contains(self, points):
        return _mesh_inside_and_distance(self.mesh, self._points(points))[1].cpu().numpy()


_TILE_ORDERS = {}


def _tile_order(H, W, device):
    """the pixels of an (H, W) image, row-major indices, listed 8 x 8 tile by tile (cached per size and device)"""
    key = (H, W, str(device))
    if key not in _TILE_ORDERS:
        r, c = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing='ij')
        rank = ((r // 8) * ((W + 7) // 8) + c // 8) * 64 + (r % 8) * 8 + c % 8
        _TILE_ORDERS[key] = torch.argsort(rank.reshape(-1))
    return _TILE_ORDERS[key]


def render_mesh_depth(mesh, R_world_cam, t_world_cam, cam, H=None, W=None, max_dist=5e1, normals=False):
    """Depth image of a triangle mesh seen by the pinhole ``cam`` at the pose (R_world_cam (3,3), t_world_cam (3,) or (3,1)):
    the sibling of ``render_depth`` with the same rays (utils_sample.ray_dirs_C, row-major, unnormalised directions
    ((c-cx)/fx, (r-cy)/fy, 1)), so a field and its mesh compare pixel by pixel.  ``mesh``: a TriangleMesh, a PLY path or an
    ops.MeshIndex (build it once for many poses).  -> (depth (H,W), mask (H,W) bool[, normals (H,W,3)]): z-depth in
    metres -- the ray parameter itself, the direction having z = 1 in the camera frame -- and 0 where nothing is hit
    within ``max_dist`` metres along the ray, the "0 = no return" of a PosedSdfRgbd frame; normals=True adds the hit
    triangle's unit normal from its winding, in the world frame, zero where not hit.  The device is the MeshIndex's,
    else the pose's; on the CPU the rays go through utils_geometry.cast_rays_torch."""
    import miso_amd.grid_opt.utils.utils_sample as utils_sample
    from miso_amd import ops
    H = int(cam.H if H is None else H)
    W = int(cam.W if W is None else W)
    device = mesh.vertices.device if isinstance(mesh, ops.MeshIndex) else R_world_cam.device
    R = R_world_cam.detach().to(device=device, dtype=torch.float32).reshape(3, 3)
    t = t_world_cam.detach().to(device=device, dtype=torch.float32).reshape(1, 3)
    dirs_c = utils_sample.ray_dirs_C(1, H, W, cam.fx, cam.fy, cam.cx, cam.cy, device, 'z').reshape(-1, 3)
    dirs_w = dirs_c @ R.T
    origins = t.expand(H * W, 3).contiguous()
    with torch.no_grad():
        if origins.is_cuda:
            # a wavefront's 64 rays as an 8 x 8 pixel tile, not 64 pixels of an image row: neighbours walk the same cells
            # (640 x 480 rays: 0.70 against 0.94 ms at 10^6 triangles, 0.19 against 0.29 ms at 10^5; profiles/cast_rays.json).
            # The answer of a ray does not depend on its place in the batch.
            order = _tile_order(H, W, device)
            t_tiled, tri_tiled, normals_of = mesh_cast_rays(mesh, origins, dirs_w[order])
            t_hit, tri = torch.empty_like(t_tiled), torch.empty_like(tri_tiled)
            t_hit[order], tri[order] = t_tiled, tri_tiled
        else:
            t_hit, tri, normals_of = mesh_cast_rays(mesh, origins, dirs_w)
        mask = (tri >= 0) & (t_hit * torch.norm(dirs_c, dim=1) <= max_dist)
        depth = torch.where(mask, t_hit, torch.zeros_like(t_hit)).reshape(H, W)
        if not normals:
            return depth, mask.reshape(H, W)
        nrm = torch.where(mask[:, None], normals_of(tri), torch.zeros_like(dirs_w)).reshape(H, W, 3)
    return depth, mask.reshape(H, W), nrm
