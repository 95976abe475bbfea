"""Overlap gate of the pairwise benchmark on the GPU (replaces lib/utils.py:713-786
compute_overlap_ratio, called per pair at scripts/benchmark_pairwise_registration.py:219-220).

    ratio = max(#{p in pc_i : NN_dist(p, trans . pc_j) < r} / |pc_i|,
                #{q in pc_j : NN_dist(q, trans^-1 . pc_i) < r} / |pc_j|)

'FCGF' method (the benchmark default): both clouds are first reduced by Open3D's
VoxelDownSample(voxel_size) and r = 3 voxel_size; '3DMatch': raw points, r = 0.05.

`FragmentOverlap` downsamples and indexes the fragments of a scene once and then scores any
batch of (pair, transform) in one launch (csrc/overlap.hip); `overlap_ratio` keeps the
reference's one-pair signature.  Geometry is fp64 like the reference's numpy/sklearn path."""
import numpy as np
import torch

from lib import _native as N

R_3DMATCH = 0.05
MAX_VOXELS_PER_AXIS = 65535   # largest 16-bit voxel index of mvr_voxel_centroids (include/mvreg.h)


def _radius(method, voxel_size):
    if method == "FCGF":
        return 3.0 * voxel_size
    if method == "3DMatch":
        return R_3DMATCH
    raise ValueError("Wrong overlap computation method was selected: %r" % (method,))


MAX_KNN = 64   # the largest k of mvr_knn_self (include/mvreg.h)


def _knn_arguments(k):
    """knn's check that needs no device -> k"""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_KNN:
        raise ValueError("knn: k must be an integer in [1, %d], not %r" % (MAX_KNN, k))
    return int(k)


def _statistical_arguments(nb_neighbors, std_ratio):
    """statistical_outliers' checks that need no device -> (nb_neighbors, std_ratio)"""
    if isinstance(nb_neighbors, bool) or int(nb_neighbors) != nb_neighbors or not 1 <= int(nb_neighbors) <= MAX_KNN:
        raise ValueError("statistical_outliers: nb_neighbors must be an integer in [1, %d], not %r"
                         % (MAX_KNN, nb_neighbors))
    if not float(std_ratio) > 0.0:
        raise ValueError("statistical_outliers: std_ratio must be positive, not %r" % (std_ratio,))
    return int(nb_neighbors), float(std_ratio)


def _ball_radius(name, radius, r, show="%g"):
    """The check of a ball's radius against r, the index's cell size, that every walk of a ball makes -> the radius as
    a float.  name: 'entry: argument'; show: how the message prints the value"""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.floating, np.integer)) \
            or not 0.0 < float(radius) <= r:
        raise ValueError(("%s " + show + " must lie in (0, %g], the index's cell size (build the FragmentOverlap with "
                          "radius >= it)") % (name, radius, r))
    return float(radius)


def _point_tensor(name, what, x, shape, xyz, show=None):
    """The check of a per-point input fo.`what` of a native call: a contiguous fp64 tensor of `shape` on the device of
    fo.xyz (`xyz`).  show: how the message prints the shape (None: without spaces)"""
    if not torch.is_tensor(x) or tuple(x.shape) != tuple(shape) or x.dtype != torch.float64 or \
            x.device != xyz.device or not x.is_contiguous():
        raise ValueError("%s: fo.%s must be a contiguous fp64 %s tensor on the device of fo.xyz"
                         % (name, what, show or "[%s]" % ",".join(str(n) for n in shape)))


def _radius_outlier_arguments(nb_points, radius, r):
    """radius_outliers' checks that need no device, r the index's cell size -> (nb_points, radius)"""
    if isinstance(nb_points, bool) or int(nb_points) != nb_points or int(nb_points) < 0:
        raise ValueError("radius_outliers: nb_points must be a non-negative integer, not %r" % (nb_points,))
    return int(nb_points), _ball_radius("radius_outliers: radius", float(r if radius is None else radius), r)


def _dbscan_arguments(eps, min_points, r):
    """cluster_dbscan's checks that need no device, r the index's cell size -> (eps, min_points); eps None: r"""
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 1 <= int(min_points) \
            <= 0x7fffffff:
        raise ValueError("cluster_dbscan: min_points must be a positive integer, not %r" % (min_points,))
    if eps is not None and isinstance(eps, (float, np.floating)) and not np.isfinite(eps):
        raise ValueError("cluster_dbscan: eps must be finite, not %r" % (eps,))
    return _ball_radius("cluster_dbscan: eps", r if eps is None else eps, r, "%r"), int(min_points)


def _cluster_keep_arguments(min_size, largest):
    """cluster_keep's checks that need no device -> (min_size or None, largest): exactly one of the two rules"""
    if not isinstance(largest, (bool, np.bool_)):
        raise ValueError("cluster_keep: largest must be True or False, not %r" % (largest,))
    if (min_size is None) == (not largest):
        raise ValueError("cluster_keep: give min_size or largest=True, one of the two")
    if min_size is not None and (isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer))
                                 or not 1 <= int(min_size) <= 0x7fffffff):
        raise ValueError("cluster_keep: min_size must be a positive integer, not %r" % (min_size,))
    return None if min_size is None else int(min_size), bool(largest)


ISS_DEFAULTS = {"salient_radius": None, "non_max_radius": None, "gamma_21": 0.975, "gamma_32": 0.975,
                "min_neighbors": 5, "min_ratio": 1e-6}


def _iss_arguments(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, min_ratio, r):
    """iss_keypoints' checks that need no device, r the index's cell size -> (salient_radius, non_max_radius,
    gamma_21, gamma_32, min_neighbors, min_ratio) with the defaults filled in (salient r, non-max 2/3 r: Open3D's
    6 : 4 ratio)"""
    r = float(r)
    radii = [_ball_radius("iss_keypoints: " + name, default if v is None else v, r, "%r")
             for name, v, default in (("salient_radius", salient_radius, r), ("non_max_radius", non_max_radius,
                                                                              2.0 * r / 3.0))]
    gammas = []
    for name, v in (("gamma_21", gamma_21), ("gamma_32", gamma_32)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 0.0 < float(v) <= 1.0:
            raise ValueError("iss_keypoints: %s must lie in (0, 1], not %r" % (name, v))
        gammas.append(float(v))
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or int(min_neighbors) < 1 \
            or int(min_neighbors) > 0x7fffffff:
        raise ValueError("iss_keypoints: min_neighbors must be a positive integer, not %r" % (min_neighbors,))
    if isinstance(min_ratio, bool) or not isinstance(min_ratio, (int, float, np.floating, np.integer)) \
            or not 0.0 <= float(min_ratio) < 1.0:
        raise ValueError("iss_keypoints: min_ratio must lie in [0, 1), not %r" % (min_ratio,))
    return radii[0], radii[1], gammas[0], gammas[1], int(min_neighbors), float(min_ratio)


def _color_rows(colors, n_raw):
    """FragmentOverlap's check of `colors` that needs no device -> a list of fp64 [n_b,3] host tensors in [0, 1]:
    uint8 values are divided by 255, float values taken as they are"""
    if len(colors) != len(n_raw):
        raise ValueError("FragmentOverlap: colors must hold one array per fragment (%d, not %d)"
                         % (len(n_raw), len(colors)))
    out = []
    for b, c in enumerate(colors):
        c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c).cpu()
        if c.dim() != 2 or tuple(c.shape) != (int(n_raw[b]), 3):
            raise ValueError("FragmentOverlap: colors[%d] must be [%d,3], one row per point, not %s"
                             % (b, int(n_raw[b]), list(c.shape)))
        if c.dtype == torch.uint8:
            c = c.to(torch.float64) / 255.0
        elif not c.is_floating_point():
            raise ValueError("FragmentOverlap: colors must be uint8 or float, not %s"
                             % str(c.dtype).replace("torch.", ""))
        out.append(c.to(torch.float64))
    return out


def _keep_mask(keep, M):
    """select's check of its mask -> a bool tensor [M] (on whatever device keep was)"""
    keep = torch.as_tensor(np.asarray(keep) if not torch.is_tensor(keep) else keep)
    if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (M,):
        raise ValueError("select: keep must be a bool / uint8 [%d], not %s %s"
                         % (M, str(keep.dtype).replace("torch.", ""), list(keep.shape)))
    return keep.bool()


class FragmentOverlap(object):
    """Downsampled (method 'FCGF') or raw ('3DMatch') fragments of a scene with a radius index on the
    GPU.  xyz_list: list of [n_b, 3] arrays / tensors (any float dtype).  radius: the index's cell size and the
    match radius instead of the method's (lib.icp refines on an index whose cells cover its search ball).
    colors: None, or a list of [n_b, 3] arrays, float in [0, 1] or uint8 (divided by 255): fo.colors is then fp64
    [M,3] on the device in the row order of fo.xyz, for 'FCGF' the mean of each voxel's colours (Open3D's
    voxel_down_sample; the colours pass through float32 there, as the points do)."""

    def __init__(self, xyz_list, method="FCGF", voxel_size=0.025, device=None, radius=None, colors=None):
        N.require_hip()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.method, self.voxel_size, self.r = method, float(voxel_size), _radius(method, voxel_size)
        if radius is not None:
            self.r = float(radius)
        L = N.lib()
        B = len(xyz_list)
        pts = [torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x) for x in xyz_list]
        n_raw = np.array([int(p.shape[0]) for p in pts], dtype=np.int64)
        off_raw = np.concatenate([[0], np.cumsum(n_raw)]).astype(np.int64)
        if colors is not None:
            colors = _color_rows(colors, n_raw)
        self.colors = None
        if method == "FCGF":
            xyz = torch.cat([p.reshape(-1, 3).to(dev, torch.float32) for p in pts]).contiguous()
            off_dev = torch.from_numpy(off_raw).to(dev)
            n = int(off_raw[-1])
            ws_b = L.mvr_voxel_centroids_workspace_bytes(n)
            ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
            cent = torch.empty(max(n, 1), 3, dtype=torch.float64, device=dev)
            off = torch.empty(B + 1, dtype=torch.int64, device=dev)
            if colors is None:
                N.check(L.mvr_voxel_centroids(N.ptr(xyz), N.ptr(off_dev), B, n, self.voxel_size, N.ptr(ws), ws_b,
                                              N.ptr(cent), N.ptr(off), N.stream()), "mvr_voxel_centroids")
            else:
                rgb = torch.cat([c.to(dev, torch.float32) for c in colors]).contiguous()
                mean = torch.empty(max(n, 1), 3, dtype=torch.float64, device=dev)
                N.check(L.mvr_voxel_centroids_colored(N.ptr(xyz), N.ptr(off_dev), B, n, self.voxel_size, N.ptr(ws),
                                                      ws_b, N.ptr(rgb), N.ptr(cent), N.ptr(off), N.ptr(mean),
                                                      N.stream()), "mvr_voxel_centroids_colored")
            self.off = off.cpu().numpy()
            if self.off[-1] < 0:    # set on the device by mvr_voxel_centroids: no synchronisation beyond this copy
                raise ValueError("FragmentOverlap: a fragment spans more than %d voxels of size %g along an axis "
                                 "(voxel indices are 16-bit, so an extent of at most %g); use a larger voxel_size"
                                 % (MAX_VOXELS_PER_AXIS, self.voxel_size, MAX_VOXELS_PER_AXIS * self.voxel_size))
            self.xyz = cent[:int(self.off[-1])].contiguous()
            if colors is not None:
                self.colors = mean[:int(self.off[-1])].contiguous()
        else:
            self.xyz = torch.cat([p.reshape(-1, 3).to(dev, torch.float64) for p in pts]).contiguous()
            self.off = off_raw
            if colors is not None:
                self.colors = torch.cat([c.to(dev) for c in colors]).reshape(-1, 3).contiguous()
        self.device = dev
        self._build_index()

    def _build_index(self):
        """What follows from xyz, off, r and device: B, M, off_dev, max_points and the radius index; what depends on
        neighbourhoods starts out None"""
        self.B, self.M = len(self.off) - 1, int(self.off[-1])
        self.off_dev = torch.from_numpy(self.off).to(self.device)
        self.max_points = int(np.max(np.diff(self.off))) if self.B else 0
        ib = N.lib().mvr_radius_index_bytes(self.M)
        self.index = torch.empty(ib, dtype=torch.uint8, device=self.device)
        N.check(N.lib().mvr_radius_index_build(N.ptr(self.xyz), *self._fragments(), N.ptr(self.index), ib, N.stream()),
                "mvr_radius_index_build")
        self.normals = self.n_nbr = None   # set by estimate_normals, or normals assigned by the caller
        self.fpfh = None                   # set by compute_fpfh
        self.intensity = self.color_grad = self.color_n_nbr = None   # set by compute_color_gradients

    def _points(self):
        """the leading arguments of a native call on the index: index, index_bytes, xyz"""
        return N.ptr(self.index), self.index.numel(), N.ptr(self.xyz)

    def _fragments(self):
        """the arguments that follow them (after the per-point inputs of the call, if any): off, B, M, r_index"""
        return N.ptr(self.off_dev), self.B, self.M, self.r

    def _kept(self, keep):
        """keep bool [M] on the device -> (rows int64 [K], the kept rows ascending, on the device; numpy int64 [B+1],
        the prefix sums of the kept points per fragment)"""
        kept_before = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), keep.long().cumsum(0)])
        return torch.nonzero(keep).reshape(-1), kept_before.cpu().numpy()[self.off].astype(np.int64)

    def estimate_normals(self, radius=None, viewpoints=None):
        """Per-point normals of every fragment (csrc/normals.hip mvr_estimate_normals: Open3D's estimate_normals with
        a radius search, restated): the eigenvector of the smallest eigenvalue of the covariance of the points of the
        same fragment closer than `radius` (None: fo.r; at most fo.r), (0, 0, 1) below three of them.
        viewpoints [B,3] (one per fragment): normals point towards them; None: the sign is unspecified.
        Stores and returns fo.normals (fp64 [M,3], device, the row order of fo.xyz); fo.n_nbr (int32 [M]) holds the
        neighbour counts."""
        radius = _ball_radius("estimate_normals: radius", float(self.r if radius is None else radius), self.r)
        vp = None
        if viewpoints is not None:
            vp = torch.as_tensor(np.asarray(viewpoints) if not torch.is_tensor(viewpoints) else viewpoints)
            if tuple(vp.shape) != (self.B, 3) or not vp.is_floating_point():
                raise ValueError("estimate_normals: viewpoints must be a float [%d,3], one per fragment" % self.B)
            vp = vp.to(self.device, torch.float64).contiguous()
        normals = torch.empty(self.M, 3, dtype=torch.float64, device=self.device)
        n_nbr = torch.empty(self.M, dtype=torch.int32, device=self.device)
        N.check(N.lib().mvr_estimate_normals(*self._points(), *self._fragments(), radius, N.ptr(vp), N.ptr(normals),
                                             N.ptr(n_nbr), N.stream()), "mvr_estimate_normals")
        self.normals, self.n_nbr = normals, n_nbr
        return normals

    def compute_fpfh(self, radius=None):
        """FPFH descriptors of every point (csrc/fpfh.hip mvr_compute_fpfh: Open3D's compute_fpfh_feature with a radius
        search, restated; the semantics are in include/mvreg.h) over the neighbours of the same fragment closer than
        `radius` (None: fo.r; at most fo.r).  Needs fo.normals (from estimate_normals or assigned by the caller);
        their sign matters, so orient them, e.g. with estimate_normals(viewpoints=...).
        Stores and returns fo.fpfh (fp32 [M,33], device, the row order of fo.xyz)."""
        radius = _ball_radius("compute_fpfh: radius", float(self.r if radius is None else radius), self.r)
        nrm = self.normals
        if nrm is None:
            raise ValueError("compute_fpfh: needs fo.normals (call fo.estimate_normals(viewpoints=...))")
        _point_tensor("compute_fpfh", "normals", nrm, (self.M, 3), self.xyz)
        L = N.lib()
        fpfh = torch.empty(self.M, 33, dtype=torch.float32, device=self.device)
        ws_b = L.mvr_compute_fpfh_workspace_bytes(self.M)
        ws = N.workspace(ws_b, self.device)
        N.check(L.mvr_compute_fpfh(*self._points(), N.ptr(nrm), *self._fragments(), radius, N.ptr(fpfh), None,
                                   N.ptr(ws), ws_b, N.stream()), "mvr_compute_fpfh")
        self.fpfh = fpfh
        return fpfh

    def compute_color_gradients(self, radius=None):
        """Per-point intensity and its gradient in the tangent plane (csrc/color_grad.hip mvr_color_gradient: what
        Open3D's registration_colored_icp prepares on its target, restated; the semantics are in include/mvreg.h) over
        the neighbours of the same fragment closer than `radius` (None: fo.r; at most fo.r).  Needs fo.colors (the
        constructor's `colors`) and fo.normals (from estimate_normals or assigned by the caller; their sign does not
        matter).  Stores fo.intensity (fp64 [M]), fo.color_grad (fp64 [M,3]) and fo.color_n_nbr (int32 [M], the
        neighbour counts), device, the row order of fo.xyz, and returns them as a dict of intensity, grad and
        n_nbr."""
        radius = _ball_radius("compute_color_gradients: radius", float(self.r if radius is None else radius), self.r)
        if self.colors is None:
            raise ValueError("compute_color_gradients: needs fo.colors (build the FragmentOverlap with colors=...)")
        nrm = self.normals
        if nrm is None:
            raise ValueError("compute_color_gradients: needs fo.normals (call fo.estimate_normals())")
        for what, x in (("normals", nrm), ("colors", self.colors)):
            _point_tensor("compute_color_gradients", what, x, (self.M, 3), self.xyz)
        intensity = torch.empty(self.M, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.M, 3, dtype=torch.float64, device=self.device)
        n_nbr = torch.empty(self.M, dtype=torch.int32, device=self.device)
        N.check(N.lib().mvr_color_gradient(*self._points(), N.ptr(nrm), N.ptr(self.colors), *self._fragments(), radius,
                                           N.ptr(intensity), N.ptr(grad), N.ptr(n_nbr), N.stream()),
                "mvr_color_gradient")
        self.intensity, self.color_grad, self.color_n_nbr = intensity, grad, n_nbr
        return {"intensity": intensity, "grad": grad, "n_nbr": n_nbr}

    def knn(self, k):
        """The k nearest points of every point within its own fragment, the point itself among them (csrc/knn_self.hip
        mvr_knn_self: Open3D's KDTreeFlann.search_knn_vector_3d on a fragment's own cloud, restated; exact).
        -> (idx int32 [M,k], dist2 fp64 [M,k]) on the device, in the row order of fo.xyz: rows of fo.xyz ordered by
        (squared distance, row); -1 / +inf beyond the fragment's size."""
        k = _knn_arguments(k)
        L = N.lib()
        idx = torch.empty(self.M, k, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(self.M, k, dtype=torch.float64, device=self.device)
        ws_b = L.mvr_knn_self_workspace_bytes(self.M)
        ws = N.workspace(ws_b, self.device)
        N.check(L.mvr_knn_self(*self._points(), *self._fragments(), k, N.ptr(idx), N.ptr(dist2), N.ptr(ws), ws_b,
                               N.stream()), "mvr_knn_self")
        return idx, dist2

    def statistical_outliers(self, nb_neighbors=20, std_ratio=2.0):
        """Open3D's remove_statistical_outlier(nb_neighbors, std_ratio) per fragment, restated (csrc/outlier.hip
        mvr_statistical_outlier): a point is kept when the mean distance to its nb_neighbors nearest points (itself
        among them, as in Open3D) lies below its fragment's mean + std_ratio standard deviations of that quantity.
        Fragments of fewer than two points keep them.  -> {"keep": bool [M], "mean_dist": fp64 [M],
        "threshold": fp64 [B]} on the device; fo.select(keep) applies it."""
        k, std_ratio = _statistical_arguments(nb_neighbors, std_ratio)
        _, dist2 = self.knn(k)
        keep = torch.empty(self.M, dtype=torch.uint8, device=self.device)
        mean_dist = torch.empty(self.M, dtype=torch.float64, device=self.device)
        thr = torch.full((self.B,), float("inf"), dtype=torch.float64, device=self.device)
        N.check(N.lib().mvr_statistical_outlier(N.ptr(dist2), N.ptr(self.off_dev), self.B, self.M, k, std_ratio,
                                                N.ptr(keep), N.ptr(mean_dist), N.ptr(thr), N.stream()),
                "mvr_statistical_outlier")
        return {"keep": keep.bool(), "mean_dist": mean_dist, "threshold": thr}

    def radius_outliers(self, nb_points=16, radius=None):
        """Open3D's remove_radius_outlier(nb_points, radius) per fragment, restated (csrc/outlier.hip
        mvr_radius_count): a point is kept when more than nb_points points of its fragment, itself among them, lie
        closer than `radius` (None: fo.r; at most fo.r).  -> {"keep": bool [M], "count": int32 [M]} on the device."""
        nb_points, radius = _radius_outlier_arguments(nb_points, radius, self.r)
        count = torch.empty(self.M, dtype=torch.int32, device=self.device)
        N.check(N.lib().mvr_radius_count(*self._points(), *self._fragments(), radius, N.ptr(count), N.stream()),
                "mvr_radius_count")
        return {"keep": count > nb_points, "count": count}

    def cluster_dbscan(self, eps=None, min_points=10):
        """Open3D's cluster_dbscan(eps, min_points) per fragment, restated (csrc/dbscan.hip mvr_cluster_dbscan; the
        semantics are in include/mvreg.h): a point is core when at least min_points points of its fragment, itself
        among them, lie closer than eps (None: fo.r; at most fo.r); a cluster is a connected component of the core
        points, numbered per fragment from 0 by its smallest core row; any other point takes the lowest-numbered
        cluster among its core neighbours, or -1 (noise).
        -> {"labels": int32 [M], "sizes": int32 [M] (sizes[fo.off[b] + c]: the points of cluster c of fragment b, 0
        beyond its clusters), "core": bool [M]} on the device and "n_clusters": numpy int64 [B]; cluster_keep turns
        them into a mask for fo.select."""
        eps, min_points = _dbscan_arguments(eps, min_points, self.r)
        L = N.lib()
        labels = torch.empty(self.M, dtype=torch.int32, device=self.device)
        sizes = torch.empty(self.M, dtype=torch.int32, device=self.device)
        core = torch.empty(self.M, dtype=torch.uint8, device=self.device)
        n_clusters = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        ws_b = L.mvr_dbscan_workspace_bytes(self.M)
        ws = N.workspace(ws_b, self.device)
        N.check(L.mvr_cluster_dbscan(*self._points(), *self._fragments(), eps, min_points, N.ptr(labels),
                                     N.ptr(n_clusters), N.ptr(sizes), N.ptr(core), N.ptr(ws), ws_b, N.stream()),
                "mvr_cluster_dbscan")
        return {"labels": labels, "n_clusters": n_clusters.cpu().numpy().astype(np.int64), "sizes": sizes,
                "core": core.bool()}

    def cluster_keep(self, clusters, min_size=None, largest=False):
        """The mask of a cluster filter from cluster_dbscan's dict -> bool [M] on the device, for fo.select: the
        points of the clusters with at least min_size points, or with largest=True of each fragment's largest cluster
        (on a tie the lowest number; Open3D users' "keep the largest cluster").  Noise is never kept.  Computed on the
        device from labels and sizes."""
        min_size, largest = _cluster_keep_arguments(min_size, largest)
        labels, sizes = clusters["labels"], clusters["sizes"]
        for what, x in (("labels", labels), ("sizes", sizes)):
            if not torch.is_tensor(x) or tuple(x.shape) != (self.M,) or x.dtype != torch.int32 or \
                    x.device != self.xyz.device:
                raise ValueError("cluster_keep: clusters[%r] must be an int32 [%d] tensor on the device of fo.xyz"
                                 % (what, self.M))
        n_b = torch.from_numpy(np.diff(self.off)).to(self.device)
        frag = torch.repeat_interleave(torch.arange(self.B, device=self.device), n_b, output_size=self.M)
        first = self.off_dev[frag]                               # the first row of each row's fragment
        labelled = labels >= 0
        if not largest:
            return labelled & (sizes[first + labels.clamp(min=0)] >= min_size)
        number = torch.arange(self.M, device=self.device) - first     # row off[b] + c holds the size of cluster c
        top = torch.zeros(self.B, dtype=torch.int32, device=self.device).scatter_reduce(0, frag, sizes, "amax")
        best = torch.full((self.B,), self.M, dtype=torch.int64, device=self.device).scatter_reduce(
            0, frag, torch.where(sizes == top[frag], number, torch.full_like(number, self.M)), "amin")
        return labelled & (labels == best[frag])

    def iss_keypoints(self, salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                      min_ratio=1e-6):
        """Open3D's compute_iss_keypoints per fragment, restated (csrc/iss.hip mvr_iss_saliency + mvr_radius_nms;
        the semantics are in include/mvreg.h).  With l1 >= l2 >= l3 the eigenvalues of the covariance of the points
        closer than salient_radius (None: fo.r), a point is a candidate with saliency l3 when it has at least
        min_neighbors of them, l2 < gamma_21 l1, l3 < gamma_32 l2 and l3 > min_ratio l1 (0: Open3D's rule; the default
        keeps rounding noise on planes from deciding); a candidate is a keypoint when no point closer than
        non_max_radius (None: 2/3 fo.r) has a larger saliency (ties: the lower row; Open3D keeps both) and that ball
        holds at least min_neighbors points.  Both radii at most fo.r.
        -> {"keep": bool [M], "saliency": fp64 [M] (-1 where not a candidate), "n_nbr": int32 [M], "rows": int64 [K]
        the kept rows of fo.xyz ascending (all on the device), "off": numpy int64 [B+1] the prefix sums of the
        keypoints per fragment}; fo.select(keep) applies it."""
        sal_r, nms_r, g21, g32, min_n, min_ratio = _iss_arguments(salient_radius, non_max_radius, gamma_21, gamma_32,
                                                                  min_neighbors, min_ratio, self.r)
        L = N.lib()
        saliency = torch.empty(self.M, dtype=torch.float64, device=self.device)
        n_nbr = torch.empty(self.M, dtype=torch.int32, device=self.device)
        keep = torch.empty(self.M, dtype=torch.uint8, device=self.device)
        N.check(L.mvr_iss_saliency(*self._points(), *self._fragments(), sal_r, g21, g32, min_ratio, min_n,
                                   N.ptr(saliency), N.ptr(n_nbr), N.stream()), "mvr_iss_saliency")
        N.check(L.mvr_radius_nms(*self._points(), *self._fragments(), nms_r, min_n, N.ptr(saliency), N.ptr(keep),
                                 N.stream()), "mvr_radius_nms")
        keep = keep.bool()
        rows, off = self._kept(keep)
        return {"keep": keep, "saliency": saliency, "n_nbr": n_nbr, "rows": rows, "off": off}

    def select(self, keep):
        """A new FragmentOverlap over the rows with keep[i] (bool / uint8 [M], array or tensor), in their order: the
        same method, voxel_size, r and device, `off` recomputed, the index rebuilt (no voxel pass), normals, n_nbr,
        fpfh and the colour gradients None since the neighbourhoods changed; colors are the kept rows' (they do not
        depend on neighbourhoods).  parent_rows (int64 [M'], device) maps its rows to this object's.
        A fragment may become empty."""
        keep = _keep_mask(keep, self.M).to(self.device)
        rows, off = self._kept(keep)
        fo = object.__new__(FragmentOverlap)
        fo.method, fo.voxel_size, fo.r, fo.device = self.method, self.voxel_size, self.r, self.device
        fo.xyz, fo.off = self.xyz[rows].contiguous(), off
        fo._build_index()
        fo.colors = None if self.colors is None else self.colors[rows].contiguous()
        fo.parent_rows = rows
        return fo

    def counts(self, pairs, trans):
        """pairs [P, 2] fragment indices, trans [P, 4, 4] (the `trans` argument of the reference) ->
        int [P, 2] matched query points (pc_i side, pc_j side)."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        trans = np.asarray(trans, dtype=np.float64).reshape(-1, 4, 4)
        P = pairs.shape[0]
        T = np.empty((P, 2, 3, 4), np.float64)
        for k in range(P):
            T[k, 0] = np.linalg.inv(trans[k])[:3]   # pc_i mapped into the frame of pc_j
            T[k, 1] = trans[k][:3]                  # pc_j mapped into the frame of pc_i
        gp = torch.from_numpy(pairs).to(self.device)
        gT = torch.from_numpy(T).to(self.device)
        cnt = torch.empty(max(P, 1), 2, dtype=torch.int32, device=self.device)
        N.check(N.lib().mvr_radius_overlap_count(*self._points(), *self._fragments()[:3], N.ptr(gp), N.ptr(gT), P,
                                                 self.max_points, self.r, N.ptr(cnt), N.stream()),
                "mvr_radius_overlap_count")
        return cnt[:P].cpu().numpy()

    def ratios(self, pairs, trans):
        """-> float64 [P]: max of the two overlap ratios (utils.py:779-786).  A pair with an empty fragment has no
        overlap: 0.0 (the reference divides by zero there)."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        c = self.counts(pairs, trans).astype(np.float64)
        n = np.diff(self.off).astype(np.float64)
        ni, nj = n[pairs[:, 0]], n[pairs[:, 1]]
        ok = (ni > 0) & (nj > 0)
        # counts are 0 beside an empty fragment, so a denominator of 1 there gives the 0.0
        return np.where(ok, np.maximum(c[:, 0] / np.where(ok, ni, 1.0), c[:, 1] / np.where(ok, nj, 1.0)), 0.0)


def overlap_ratio(pc_i, pc_j, trans, method="3DMatch", voxel_size=0.025):
    """utils.py:713 compute_overlap_ratio(pc_i, pc_j, trans, method, voxel_size) for one pair."""
    fo = FragmentOverlap([pc_i, pc_j], method, voxel_size)
    return float(fo.ratios([[0, 1]], [trans])[0])
