"""Seeded inputs of the reference-pinned sphere-tracing golden (tests/golden/sphere_trace.npz, written by
tools/make_goldens.py: gen_sphere_trace with the reference's own sphere_tracing on the reference's GridNet).

The scene is a real distance field, so that tracing converges: min(sphere, floor plane, tilted wall), evaluated at the
voxel centres of every level and stored as value / n_levels in channel 0 of that level (all other features zero).  The
decoder passes the sum of those channels through exactly: W0 rows +e and -e, the identity on those two hidden units,
output h0 - h1, no bias -- relu(v) - relu(-v) = v.  The field a model built from this returns is therefore the mean over
the levels of the trilinear interpolant of the scene.

Pure numpy + the model handed in: the reference's GridNet and the mirror's are baked by the same code."""
import numpy as np

GRID = dict(bound=[[-1.0, 1.0], [-0.75, 0.75], [-1.0, 1.0]], base_cell=0.25, scale=2, n_levels=3, fdim=8, hidden=64)

SPHERE_C, SPHERE_R = np.array([0.2, -0.2, 0.3]), 0.3
FLOOR_Y = -0.55
WALL_N = np.array([-0.25, 0.1, -1.0]) / np.linalg.norm([-0.25, 0.1, -1.0])
WALL_P = np.array([0.0, 0.0, 0.8])

# The golden's rays: 768 from one pinhole at `eye`, directions ((c - cx) / fx, (r - cy) / fy, 1) in the camera frame --
# not unit length -- in two bundles of 384 (golden_rays): the upper half of the image of CAMERA, which looks down on the
# floor almost along its normal, and the lower half of the image of the same camera turned to CAMERA_FREE's look_at,
# into free space where nothing lies within max_dist.  The floor bundle starts inside the part of the grid where the
# interpolant is the scene exactly (a plane is reproduced by trilinear interpolation; away from the half cell at the
# bound, closer to the floor than to the sphere): a ray is still moving after one iteration, lands within 1e-4 of the
# surface in two steps and no field value comes near epsilon.  The free bundle walks on until it is far.  Generic
# views of a surface do not stay clear of epsilon -- a ray meeting it at angle a converges by 1 - cos a per step, so
# its values cross the 2e-5 band around epsilon with probability ~0.4 / ln(1 / (1 - cos a)); from VIEW below 22.5 % of
# the rays are marginal by the generator's definition (tools/make_goldens.py), against the 2 % it admits.
CAMERA = dict(eye=[-0.6, 0.5, -0.6], look_at=[-0.58, -0.55, -0.57], H=24, W=32, fx=229.0, fy=229.0, cx=15.5, cy=11.5)
CAMERA_FREE = dict(CAMERA, look_at=[1.0, 0.5, 1.0])
# A view of the whole scene (sphere, floor, free space beyond max_dist, rays still moving at the cut-off): what
# render_depth is checked on against the analytic scene.
VIEW = dict(eye=[-0.6, 0.3, -0.7], look_at=[0.2, -0.2, 0.3], H=24, W=32, fx=40.0, fy=40.0, cx=15.5, cy=11.5)
TRACE = dict(epsilon=1e-4, min_dist=1e-3, max_dist=1.5)
# max_iters of the golden runs: the two long ones, and short ones that stop rays on their way (after one iteration every
# ray is still moving: no hit, no far ray yet)
RUNS = (100, 12, 3, 2, 1)


def scene_sdf(p):
    """(N,3) float64 -> (N,) signed distance to min(sphere, floor, wall), positive on the camera's side."""
    p = np.asarray(p, dtype=np.float64)
    sphere = np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R
    floor = p[..., 1] - FLOOR_Y
    wall = (p - WALL_P) @ WALL_N
    return np.minimum(np.minimum(sphere, floor), wall)


def scene_ray_distance(origins, dirs_unit):
    """Distance along each unit ray to the scene's surface (float64; inf where the ray meets none of the three)."""
    o, d = np.asarray(origins, dtype=np.float64), np.asarray(dirs_unit, dtype=np.float64)
    inf = np.full(o.shape[0], np.inf)
    oc = o - SPHERE_C
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - SPHERE_R ** 2)
    root = -b - np.sqrt(np.where(disc > 0, disc, 0.0))
    t_sphere = np.where((disc > 0) & (root > 0), root, inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = (FLOOR_Y - o[:, 1]) / d[:, 1]
        tw = ((WALL_P - o) @ WALL_N) / (d @ WALL_N)
    t_floor = np.where((d[:, 1] < 0) & (tf > 0), tf, inf)
    t_wall = np.where(((d @ WALL_N) < 0) & (tw > 0), tw, inf)
    return np.minimum(np.minimum(t_sphere, t_floor), t_wall)


def camera_pose(cam=None):
    """R_world_cam (3,3) with columns (right, down, forward) and t_world_cam (3,), float64."""
    cam = CAMERA if cam is None else cam
    eye = np.asarray(cam["eye"], dtype=np.float64)
    fwd = np.asarray(cam["look_at"], dtype=np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack((right, down, fwd), axis=1), eye


def rays(cam=None):
    """(origins (N,3), directions (N,3)) float32, row-major over the image; directions are not normalised."""
    cam = CAMERA if cam is None else cam
    R, eye = camera_pose(cam)
    r, c = np.meshgrid(np.arange(cam["H"], dtype=np.float64), np.arange(cam["W"], dtype=np.float64), indexing="ij")
    dc = np.stack(((c - cam["cx"]) / cam["fx"], (r - cam["cy"]) / cam["fy"], np.ones_like(c)), axis=-1).reshape(-1, 3)
    dw = dc @ R.T
    return np.broadcast_to(eye, dw.shape).astype(np.float32).copy(), dw.astype(np.float32)


def golden_rays():
    """The golden's 768 rays: rows 0-11 of CAMERA's image, then rows 12-23 of CAMERA_FREE's."""
    half = CAMERA["H"] // 2 * CAMERA["W"]
    (o0, d0), (o1, d1) = rays(CAMERA), rays(CAMERA_FREE)
    return np.concatenate((o0[:half], o1[half:])), np.concatenate((d0[:half], d1[half:]))


def model_cfg():
    import golden_cases as gc
    g = GRID
    return gc.model_cfg(g["bound"], g["base_cell"], g["scale"], g["n_levels"], g["fdim"], g["hidden"])


def decoder_state():
    """MLPNet state dict (numpy) of the exact pass-through decoder."""
    g = GRID
    F, H, C = g["fdim"] * g["n_levels"], g["hidden"], g["fdim"]
    w0 = np.zeros((H, F), dtype=np.float32)
    w0[0, ::C] = 1.0
    w0[1, ::C] = -1.0
    w1 = np.zeros((H, H), dtype=np.float32)
    w1[0, 0] = w1[1, 1] = 1.0
    w2 = np.zeros((1, H), dtype=np.float32)
    w2[0, 0], w2[0, 1] = 1.0, -1.0
    return {"network.0.weight": w0, "network.0.bias": np.zeros(H, dtype=np.float32),
            "network.2.weight": w1, "network.2.bias": np.zeros(H, dtype=np.float32),
            "network.4.weight": w2, "network.4.bias": np.zeros(1, dtype=np.float32)}


def bake(net, sdf=scene_sdf):
    """Write the scene into the feature grids and the pass-through decoder into ``net`` (a GridNet of model_cfg(), the
    reference's or the mirror's), in place."""
    import torch
    n_levels = len(net.features)
    with torch.no_grad():
        for g in net.features:
            f = g.feature
            _, C, Z, Y, X = f.shape
            pos = g.vertex_positions().detach().cpu().double().numpy()          # (Z*Y*X, 3), z-major
            val = (sdf(pos) / n_levels).astype(np.float32).reshape(Z, Y, X)
            f.zero_()
            f[0, 0].copy_(torch.from_numpy(val).to(f))
    net.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in decoder_state().items()})
    return net
