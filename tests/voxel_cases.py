"""Seeded point clouds for the voxel down-sampling tests (tests/test_voxel_down.py) and for the tool that records what
the reference selects on them (tools/make_voxel_goldens.py -> tests/golden/voxel_down.npz, index arrays only).

Every family aims at one property of utils_geometry.voxel_down_sample_torch; none holds an input the reference itself
cannot handle (an empty cloud, every point exactly on a cell centre so that max(dist) = 0, NaN)."""
import numpy as np

ROOM_LO = np.array([-4.0, -2.5, -0.2], dtype=np.float32)
ROOM_HI = np.array([4.0, 2.5, 2.8], dtype=np.float32)


def room(n=100000, seed=7):
    """Uniform samples of an 8 x 5 x 3 m room."""
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (n, 3)).astype(np.float32) * (ROOM_HI - ROOM_LO) + ROOM_LO).astype(np.float32)


def clustered(seed=11, cells=1000, per=30, v=0.1):
    """About 30 points in each of 1000 voxels of the room: the (rank, index) contest inside a voxel."""
    rs = np.random.RandomState(seed)
    span = np.floor((ROOM_HI - ROOM_LO) / v).astype(np.int64)
    ijk = np.stack([rs.randint(0, span[a], cells) for a in range(3)], axis=1)
    ijk = np.repeat(ijk, per, axis=0)
    pts = (ijk + rs.uniform(0.02, 0.98, ijk.shape)) * v + np.floor(ROOM_LO / v) * v
    return pts[rs.permutation(pts.shape[0])].astype(np.float32)


def lattice(seed=13, n=20000):
    """Multiples of 1/16 in [0, 2)^3 with v = 0.25: every operation is exact, equal distances meet in every voxel and the
    lowest index has to win."""
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 32, (n, 3)) / 16.0).astype(np.float32)


def alias(seed=17, n=5000):
    """x spans cells 0..10 and is the longest axis, so side = 10 is an occupied x index: the reference's key of
    (10, iy, iz) equals that of (0, iy + 1, iz), and the two cells yield one point."""
    rs = np.random.RandomState(seed)
    hi = np.array([1.05, 0.6, 0.3])
    pts = rs.uniform(0, 1, (n, 3)) * hi
    pts[0] = [1.049, 0.01, 0.01]          # the extremes are present whatever the draw
    pts[1] = [0.001, 0.001, 0.001]
    return pts.astype(np.float32)


def one_voxel(seed=19, n=1000):
    rs = np.random.RandomState(seed)
    return rs.uniform(0.01, 0.09, (n, 3)).astype(np.float32)


def single():
    return np.array([[0.3, -1.2, 0.7]], dtype=np.float32)


def cases():
    """name -> (points (N,3) float32, voxel_size)"""
    r = room()
    return {"room_005": (r, 0.05),
            "room_001": (r, 0.01),            # keys beyond 2^24: neighbouring voxels merge in the fp32 key
            "clustered": (clustered(), 0.1),
            "lattice": (lattice(), 0.25),
            "alias": (alias(), 0.1),
            "one_voxel": (one_voxel(), 0.1),
            "single": (single(), 0.05)}


# --- LiDAR frames: the reference's per-frame load sequence (grid_opt/datasets/sdf_3d_lidar.py:108-133) -----------------
LIDAR = dict(voxel_size=0.5, max_range=60.0, min_range=1.5, min_z=-3.0, max_z=60.0)


def lidar_frames(seed=23):
    """Two sensor-frame scans: a wide one (the crop range stays at max_range) and a lopsided one (the sensor near a
    corner: the adaptive range drops to 12 m, the voxel size with it, and the range crop cuts points away)."""
    rs = np.random.RandomState(seed)
    out = []
    for n, lo, hi in ((3000, (-40.0, -20.0, -4.0), (40.0, 20.0, 4.0)), (2000, (-6.0, -5.0, -3.5), (30.0, 25.0, 3.0))):
        lo, hi = np.array(lo), np.array(hi)
        out.append((rs.uniform(0, 1, (n, 3)) * (hi - lo) + lo).astype(np.float32))
    return out
