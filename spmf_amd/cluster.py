"""What surrounds the library's Lloyd step (include/spmf_hip.h spmf_kmeans_step): the starting centroids, the
centroid update and the loop of ``AnalysisQueries.kmeans``.  Plain torch around one library call per
iteration; the assignment and the sums -- the hot path -- are csrc/kmeans.hip behind csrc/knn.hip.
"""
import torch

from . import _args, _lib

INITS = ("k-means++", "first")
MAX_CLUSTERS = 65536


def check_args(name, n_clusters, max_iter, init):
    """``n_clusters``, ``max_iter`` and a named ``init`` of ``kmeans`` / ``cluster``, checked before any library
    call -> (G, max_iter)."""
    if not 1 <= _args.integer(name, "n_clusters", n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"{name} needs 1 <= n_clusters <= {MAX_CLUSTERS}, got {n_clusters}")
    _args.integer(name, "max_iter", max_iter, 1)
    if not isinstance(init, torch.Tensor) and not (isinstance(init, str) and init in INITS):
        raise ValueError(f"{name}: init must be one of {INITS} or a float32 [n_clusters, width] tensor, got {init!r}")
    return int(n_clusters), int(max_iter)


def check_init_tensor(name, init, G, points):
    """A tensor ``init`` against the points it starts from: float32 [G, width] on their device."""
    if init.dim() != 2 or tuple(init.shape) != (G, points.shape[1]):
        raise ValueError(f"{name}: an init tensor must have shape {(G, points.shape[1])}, got {tuple(init.shape)}")
    if init.dtype != torch.float32:
        raise ValueError(f"{name}: an init tensor must be float32, got {init.dtype}")
    if init.device != points.device:
        raise ValueError(f"{name}: an init tensor must be on the device of the points {points.device}, got "
                         f"{init.device}")


def _finite_rows(points):
    return torch.isfinite(points).all(dim=1)


def init_first(points, G):
    """The first ``G`` finite rows of ``points`` (fewer finite rows: a ValueError)."""
    idx = torch.nonzero(_finite_rows(points)).flatten()[:G]
    if idx.numel() < G:
        raise ValueError(f"kmeans: init='first' needs {G} finite rows, the points have {idx.numel()}")
    return points[idx].contiguous()


def init_plus_plus(points, G, seed=0):
    """k-means++ starting centres: ``G`` rows of ``points`` (float32 [N, width]) by D^2 sampling on the points'
    device.  The first centre is uniform over the finite rows; each further one is drawn with probability
    proportional to the squared distance (fp64) to the nearest centre so far, through an fp64 cumulative sum and
    ``searchsorted``.  The uniform draws come from a CPU ``torch.Generator`` seeded with ``seed``: the same seed
    gives the same centres on the same machine.  Only finite rows are eligible (none: a ValueError); when every
    eligible row coincides with a centre the next one is uniform over the eligible rows.

    Cost: a start, not a hot path -- plain torch.  It keeps an fp64 copy of the points (8 N width bytes), and each
    of the G centres takes one more fp64 temporary of that size and one host synchronisation; at 10^6 x 256 that
    is 2 GB + 2 GB.  For large N x width x G start from a subsample (``init_plus_plus(points[::stride], G)`` is a
    valid tensor ``init``) or from ``init='first'``."""
    G = int(G)
    finite = _finite_rows(points)
    if not bool(finite.any()):
        raise ValueError("init_plus_plus: no row of the points is finite")
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    u = torch.rand(G, generator=gen, dtype=torch.float64).to(points.device)
    x = torch.where(finite[:, None], points, torch.zeros_like(points)).to(torch.float64)
    eligible = finite.to(torch.float64)

    def draw(weight, ui):
        cum = torch.cumsum(weight, 0)
        i = torch.searchsorted(cum, (ui * cum[-1]).reshape(1), right=True).clamp_(max=weight.numel() - 1)
        # (a zero-weight row is never the first with cum > target, except behind the clamp: step back onto weight)
        pos = torch.nonzero(weight > 0).flatten()
        return pos[torch.searchsorted(pos, i, right=True).clamp_(min=1) - 1].reshape(())
    chosen = []
    d2 = None
    for g in range(G):
        weight = eligible if d2 is None else d2 * eligible
        if d2 is not None and not bool((weight > 0).any()):
            weight = eligible
        i = draw(weight, u[g])
        chosen.append(i)
        new = ((x - x[i]) ** 2).sum(1)
        d2 = new if d2 is None else torch.minimum(d2, new)
    return points[torch.stack(chosen)].contiguous()


def update_centroids(sums, counts, old):
    """The centroid update of one Lloyd step: ``sums`` fp64 [G, width] / ``counts`` int64 [G] in fp64, rounded
    to float32; an empty cluster keeps its row of ``old`` (float32 [G, width])."""
    n = counts.to(torch.float64).unsqueeze(1)
    mean = (sums / torch.where(n > 0, n, torch.ones_like(n))).to(torch.float32)
    return torch.where(n > 0, mean, old)


def lloyd(h, points, centroids, max_iter):
    """The loop of ``kmeans`` on the context ``h``: a step on the current centroids, stop when no label changed,
    else the update; one read-back (the three statistics) per iteration.  Every output refers to the centroids of
    the last step."""
    N, width, G = int(points.shape[0]), int(points.shape[1]), int(centroids.shape[0])
    dev = points.device
    labels = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2)]
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    sums = torch.empty(G, width, dtype=torch.float64, device=dev)
    counts = torch.empty(G, dtype=torch.int64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    scratch = (_lib.Scratch(dev), "spmf_kmeans_scratch_bytes", N, G, width)     # one buffer for every step
    centroids = centroids.contiguous()
    converged, n_iter, st = False, 0, None
    for it in range(max_iter):
        cur, prev = labels[it & 1], labels[(it & 1) ^ 1]
        _lib.call(h, "spmf_kmeans_step", points.data_ptr(), N, width, centroids.data_ptr(), G,
                  prev.data_ptr() if it else None, cur.data_ptr(), dist.data_ptr(), sums.data_ptr(),
                  counts.data_ptr(), stats.data_ptr(), device=dev, scratch=scratch)
        st = stats.tolist()                         # the iteration's one read-back
        n_iter = it + 1
        if st[1] == 0:
            converged = True
            break
        if it + 1 < max_iter:
            centroids = update_centroids(sums, counts, centroids).contiguous()
    return {"labels": labels[(n_iter - 1) & 1], "distances": dist, "centroids": centroids, "counts": counts,
            "inertia": float(st[0]), "n_iter": n_iter, "converged": converged, "n_unassigned": int(st[2])}
