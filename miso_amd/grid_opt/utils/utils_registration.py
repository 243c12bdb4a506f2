"""ICP registration: Open3D's ``registration_icp`` restated from its documented behaviour (the reference calls it from
grid_opt/utils/utils_scannet.py:115-156 and grid_opt/align/icp.py:51-118; Open3D is not a dependency here).  The per-point
work of an iteration -- transform, nearest-neighbour search, the reduction of the correspondences to 32 doubles -- runs
in HIP (ops.IcpWorkspace, csrc/icp.hip); this module is the float64 solve on the host and the loop around it.

Conventions written down where Open3D's documentation leaves them open:
  * a pair is a correspondence when its distance is ``<= max_dist`` (csrc/icp.hip compares squares);
  * ``fitness = inliers / len(src)``, ``inlier_rmse = sqrt(sum d^2 / inliers)`` (0 without inliers);
  * the loop evaluates at ``init``; an iteration solves from the current correspondences, left-multiplies the update
    onto T and evaluates again; it stops when ``|d fitness| < relative_fitness and |d rmse| < relative_rmse``, after
    ``max_iteration`` updates, or -- with the current T -- when there is no inlier or the system is singular / non-finite;
  * the Tukey loss weighs point-to-plane residuals only (Open3D's point-to-point estimate takes no kernel)."""
from dataclasses import dataclass, field

import numpy as np

from miso_amd import ops

# positions in the block of sums (csrc/icp.hip)
_COUNT, _SUM_D2, _A, _B, _WR2 = 0, 1, slice(2, 23), slice(23, 29), 29
_SUM_P, _SUM_Q, _QP = slice(2, 5), slice(5, 8), slice(8, 17)
_TRIU = np.triu_indices(6)


@dataclass
class TukeyLoss:
    """w(r) = (1 - (r / k)^2)^2 for |r| <= k, 0 beyond it (Open3D's TukeyLoss)"""
    k: float = 1e-2


@dataclass
class RegistrationResult:
    transformation: np.ndarray = field(default_factory=lambda: np.eye(4))
    fitness: float = 0.0
    inlier_rmse: float = 0.0
    iterations: int = 0

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.6e}, inlier_rmse={self.inlier_rmse:.6e}, "
                f"iterations={self.iterations})")


def tukey_weight(r, k):
    r = np.asarray(r, dtype=np.float64)
    s = r / k
    u = 1.0 - s * s
    return np.where(np.abs(r) <= k, u * u, 0.0)


def transform_vector6d_to_matrix4d(x) -> np.ndarray:
    """Open3D's TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3:6]"""
    (ca, cb, cg), (sa, sb, sg) = np.cos(x[:3]), np.sin(x[:3])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def solve_point_to_plane(sums):
    """The update of one point-to-plane iteration from the block of sums: A x = -b -> 4 x 4, or None when the system is
    singular or not finite."""
    A = np.zeros((6, 6))
    A[_TRIU] = sums[_A]
    A = A + np.triu(A, 1).T
    b = np.asarray(sums[_B], dtype=np.float64)
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None
    try:
        if np.linalg.matrix_rank(A) < 6:
            return None
        x = np.linalg.solve(A, -b)
    except np.linalg.LinAlgError:
        return None
    return transform_vector6d_to_matrix4d(x) if np.isfinite(x).all() else None


def umeyama_from_sums(count, sum_p, sum_q, sum_qp, origin=(0.0, 0.0, 0.0)):
    """Umeyama without scale from sums taken relative to ``origin``: R, t minimising sum |R p + t - q|^2.  A reflection
    (det U det V < 0) flips the axis of the smallest singular value.  -> 4 x 4, or None."""
    if not count > 0:
        return None
    o = np.asarray(origin, dtype=np.float64)
    pm, qm = np.asarray(sum_p, dtype=np.float64) / count, np.asarray(sum_q, dtype=np.float64) / count
    H = np.asarray(sum_qp, dtype=np.float64).reshape(3, 3) / count - np.outer(qm, pm)
    if not np.isfinite(H).all():
        return None
    U, _, Vt = np.linalg.svd(H)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = (qm + o) - T[:3, :3] @ (pm + o)
    return T


def converged(prev, cur, relative_fitness, relative_rmse) -> bool:
    """Open3D's ICPConvergenceCriteria on two successive (fitness, inlier_rmse) pairs"""
    return abs(prev[0] - cur[0]) < relative_fitness and abs(prev[1] - cur[1]) < relative_rmse


def _evaluation(sums, n):
    count = float(sums[_COUNT])
    return (count / n if n else 0.0), (float(np.sqrt(sums[_SUM_D2] / count)) if count > 0 else 0.0)


def estimate_normals(points, knn=30, radius=None, index=None):
    """Open3D's ``PointCloud.estimate_normals`` restated from its documented behaviour: for every point the unit
    eigenvector of the smallest eigenvalue of the covariance of its neighbours among ``points`` -- by default its
    ``knn`` = 30 nearest (KDTreeSearchParamKNN, the point itself being the first), with ``radius`` those within it
    (KDTreeSearchParamRadius; ``knn`` is then not read, Open3D's hybrid search is not built).  Fewer than three neighbours,
    or neighbours on a line, give (0, 0, 1).  Normals are NOT oriented (Open3D's are not either).  ``index``: an
    ops.NearestIndex over ``points`` to reuse, else one is built.  -> (N, 3) fp32 on the device (ops.NearestIndex.normals)."""
    index = ops.NearestIndex(points) if index is None else index
    if tuple(index.tgt.shape) != tuple(points.shape):
        raise ValueError("estimate_normals: index is not built on points")
    return index.normals(radius=radius)[0] if radius is not None else index.normals(knn=int(knn))[0]


def registration_icp(src, tgt_index, tgt=None, tgt_normals=None, max_dist=0.05, init=None, kind='point_to_plane',
                     loss=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, callback=None
                     ) -> RegistrationResult:
    """Align ``src`` (N, 3) to the cloud behind ``tgt_index`` (an ops.NearestIndex, built once and reused across calls).
    ``tgt``: the indexed cloud, if given it must be the index's own; ``tgt_normals`` (M, 3) for 'point_to_plane';
    ``loss``: None (L2) or a TukeyLoss; ``init``: 4 x 4, default the identity.  ``callback(iteration, T, fitness, rmse)``
    is called after every evaluation (iteration 0 = at ``init``).  One device-to-host read per evaluation."""
    if kind not in ops.ICP_KINDS:
        raise ValueError(f"Unknown constraint type {kind}")
    if tgt is not None and tuple(tgt.shape) != tuple(tgt_index.tgt.shape):
        raise ValueError("registration_icp: tgt is not the cloud the index was built on")
    k = None if loss is None else float(getattr(loss, "k", loss))
    work = ops.IcpWorkspace(src, tgt_index, tgt_normals)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    n = int(work.n)
    sums = work.step(T, max_dist, kind, k)
    cur = _evaluation(sums, n)
    iterations = 0
    if callback:
        callback(0, T.copy(), *cur)
    for _ in range(int(max_iteration)):
        if kind == 'point_to_plane':
            update = solve_point_to_plane(sums) if sums[_COUNT] > 0 else None
        else:
            update = umeyama_from_sums(sums[_COUNT], sums[_SUM_P], sums[_SUM_Q], sums[_QP], work.origin)
        if update is None:
            break
        T = update @ T
        iterations += 1
        prev = cur
        sums = work.step(T, max_dist, kind, k)
        cur = _evaluation(sums, n)
        if callback:
            callback(iterations, T.copy(), *cur)
        if converged(prev, cur, relative_fitness, relative_rmse):
            break
    return RegistrationResult(T, cur[0], cur[1], iterations)


def get_information_matrix(src, tgt_index, max_dist, transformation) -> np.ndarray:
    """Open3D's get_information_matrix_from_point_clouds: the 6 x 6 sum of G^T G over the correspondences of ``src`` moved
    by ``transformation`` (distance <= max_dist), G = [-[q]x, I] at the target point q.  One search, the rest a handful of
    float64 torch reductions (it runs once per pair)."""
    import torch
    moved = ops.icp_transform(src, transformation)
    d2, idx, _ = tgt_index.query(moved)
    ok = (idx >= 0) & (d2.to(torch.float64) <= float(max_dist) ** 2)
    q = tgt_index.tgt[idx[ok]].to(torch.float64)
    sq, sqq, count = q.sum(dim=0).cpu().numpy(), (q.T @ q).cpu().numpy(), int(q.shape[0])
    cross = np.array([[0.0, -sq[2], sq[1]], [sq[2], 0.0, -sq[0]], [-sq[1], sq[0], 0.0]])
    info = np.zeros((6, 6))
    info[:3, :3] = np.trace(sqq) * np.eye(3) - sqq          # sum [q]x^T [q]x
    info[:3, 3:] = cross                                    # sum (-[q]x)^T
    info[3:, :3] = cross.T
    info[3:, 3:] = count * np.eye(3)
    return info
