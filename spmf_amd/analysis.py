"""The analysis calls of the model classes on rows and graphs as given: ``AnalysisQueries`` is the mixin that gives
PoissonFactorization (and through it the Bernoulli and mixed classes) knn, kmeans, silhouette, fuzzy_graph,
graph_layout, graph_transform, spectral, spectral_cluster, communities, paga, paga_init and geodesic, and the
composites that start from ``StreamingQueries.embed``: neighbors, cluster, umap, umap_transform and pseudotime.

None of the calls here runs the draw stage: each takes float32 points [N, Kx] or a CSR graph on the model's device
(include/spmf_hip.h; csrc/api_points.hip and csrc/api_graph.hip).  A call is: the check of its arguments, which
comes first (``_args.integer`` / ``_args.number``, ``_knn_rows``, ``_graph_tensors`` / ``_graph_numbers``,
``_on_device``), its output tensors, and ``_lib.call``, the one place a library call, its scratch and its stream
are spelled.  The loops around a call are modules of their own: ``cluster`` (Lloyd), ``spectral``,
``communities``, ``paga`` and ``geodesic`` (their ``LibraryOps``), ``graph`` and ``neighbors`` (plain torch).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _args, _lib
from .streaming import _vector


class AnalysisQueries:
    """The calls on rows and graphs as given.  The host class supplies ``device``, ``latent_dim``,
    ``surrogate_distribution``, ``_custom_codec``, ``_handle`` and, from ``StreamingQueries``, ``embed`` and
    ``_label_range``."""

    @staticmethod
    def _knn_args(name, k, metric):
        """k and the metric of ``knn`` / ``neighbors``, checked before any library call -> (k, flags)."""
        from . import neighbors as _neighbors
        if not 1 <= _args.integer(name, "k", k) <= 64:
            raise ValueError(f"{name} needs 1 <= k <= 64, got {k}")
        if metric not in _neighbors.METRICS:
            raise ValueError(f"{name}: metric must be one of {_neighbors.METRICS}, got {metric!r}")
        return int(k), 1 if metric == "cosine" else 0

    @staticmethod
    def _knn_rows(name, what, t):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: {what} must be a torch tensor, got {type(t).__name__}")
        if t.dim() != 2:
            raise ValueError(f"{name}: {what} must be 2-D [rows, width], got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be float32, got {t.dtype}")
        if not 1 <= t.shape[1] <= 256:
            raise ValueError(f"{name}: the width of {what} must be in 1..256, got {t.shape[1]}")
        return t

    def _on_device(self, name, what, t):
        """``t`` (``what`` in the message: "points", "the graph") is on the model's device."""
        dev = torch.device(self.device)
        if t.device.type != "cuda" or (dev.index is not None and t.device != dev):
            raise ValueError(f"{name}: {what} must be on the model's device {self.device}, got {t.device}")

    def knn(self, points, k=15, queries=None, metric="euclidean", include_self=False):
        """The exact ``k`` nearest rows of ``points`` [Nr, Kx] for every row of ``queries`` [Nq, Kx]
        (default: ``points`` itself), without an [Nq, Nr] array (csrc/knn.hip).  Both are float32
        tensors on the model's device, 1 <= Kx <= 256 whatever the model's latent_dim, 1 <= k <= 64.
        ``metric``: 'euclidean' or 'cosine' (the distance 1 - cos).  Without ``queries`` (or with
        ``queries=points``) a row is no neighbour of its own unless ``include_self``.

        Returns {'indices': int32 [Nq,k], 'distances': float32 [Nq,k]} on the device: distance
        ascending, equal distances by ascending index, a query with fewer than k candidates padded
        with -1 / +inf at the tail.  A non-finite row of ``points`` is nobody's neighbour; a non-finite
        query (or a zero row under 'cosine') has none.  The selection runs on the matrix cores over
        centred (or unit) rows; the reported distances are recomputed from the rows as given
        (include/spmf_hip.h spmf_knn has the definition).  Bit-reproducible; a query's result does
        not depend on the other queries.  ``spmf_amd.neighbors.to_csr`` turns the result into the
        CSR arrays of a neighbour graph."""
        k, flags = self._knn_args("knn", k, metric)
        pts = self._knn_rows("knn", "points", points)
        same = queries is None or queries is points or (
            isinstance(queries, torch.Tensor) and queries.shape == points.shape and queries.dtype == points.dtype
            and queries.device == points.device and queries.data_ptr() == points.data_ptr()
            and queries.stride() == points.stride())
        qry = pts if same else self._knn_rows("knn", "queries", queries)
        if qry.shape[1] != pts.shape[1]:
            raise ValueError(f"knn: queries have width {qry.shape[1]}, points {pts.shape[1]}")
        if pts.shape[0] > 2 ** 31 - 1:
            raise ValueError(f"knn: {pts.shape[0]} points are beyond the int32 index of the result")
        self._on_device("knn", "points", pts)
        self._on_device("knn", "queries", qry)
        pts = pts.contiguous()
        qry = pts if same else qry.contiguous()
        nq, nr, width = int(qry.shape[0]), int(pts.shape[0]), int(pts.shape[1])
        idx = torch.empty(nq, k, dtype=torch.int32, device=pts.device)
        dist = torch.empty(nq, k, dtype=torch.float32, device=pts.device)
        _lib.call(self._handle(), "spmf_knn", qry.data_ptr(), nq, pts.data_ptr(), nr, width, k, flags,
                  0 if same and not include_self else -1, idx.data_ptr(), dist.data_ptr(), device=pts.device,
                  scratch=(_lib.Scratch(pts.device), "spmf_knn_scratch_bytes", nq, nr, width))
        return {"indices": idx, "distances": dist}

    def neighbors(self, data, k=15, query=None, metric="euclidean", include_self=False, nsamples=32, draws=None,
                  max_rows=None):
        """The neighbour graph of the rows of ``data`` in the model's latent space: ``embed`` on
        ``data`` -- and on ``query``, when given, with the SAME draws -- then ``knn`` on the posterior
        mean encodings.  Without ``query`` every row of ``data`` gets its k nearest other rows (itself
        too with ``include_self``); with ``query`` every row of ``query`` gets its k nearest rows of
        ``data``.  ``data`` / ``query``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed``;
        ``k`` and ``metric`` as in ``knn``.

        Returns {'indices': int32 [Nq,k], 'distances': float32 [Nq,k]} on the device, bit for bit
        ``knn(embed(data, draws=draws)["mean"], k, ...)``."""
        self._knn_args("neighbors", k, metric)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"neighbors: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        if draws is None and self._custom_codec is None:
            if int(nsamples) < 1:
                raise ValueError("neighbors needs nsamples >= 1")
            draws = self.surrogate_distribution.sample(int(nsamples))      # once: data and query share them
        ref = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        if query is None:
            return self.knn(ref, k=k, metric=metric, include_self=include_self)
        qry = self.embed(query, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        return self.knn(ref, k=k, queries=qry, metric=metric, include_self=True)

    def kmeans(self, points, n_clusters, init="k-means++", max_iter=100, seed=0):
        """Deterministic k-means (Lloyd's iteration) of the rows of ``points`` [N, Kx], a float32 tensor on the
        model's device with 1 <= Kx <= 256 whatever the model's latent_dim, into 1 <= ``n_clusters`` <= 65536
        clusters.  One library call per iteration (include/spmf_hip.h spmf_kmeans_step, csrc/kmeans.hip): the
        assignment is ``knn``'s -- the label of a row is, bit for bit,
        ``knn(centroids, k=min(4, G), queries=points)["indices"][:, 0]`` -- and the clusters' sums are fp64 in
        a fixed order, so two runs of an iteration give the same centroids.

        ``init``: 'k-means++' (``spmf_amd.cluster.init_plus_plus`` with ``seed``), 'first' (the first
        ``n_clusters`` finite rows) or a float32 [n_clusters, Kx] tensor on the device.  The loop: a step on
        the current centroids; stop when no label changed; else centroids = sums / counts in fp64 rounded to
        float32, an empty cluster keeping its centroid; at most ``max_iter`` steps.  One read-back of three
        numbers per iteration.

        Returns {'labels': int32 [N] (-1: a non-finite row), 'distances': float32 [N] (+inf beside -1),
        'centroids': float32 [G, Kx], 'counts': int64 [G]} on the device and 'inertia' (the sum of the squared
        distances), 'n_iter', 'converged', 'n_unassigned'.  Every output refers to the returned centroids, at
        ``max_iter`` too.  Bit-reproducible for a tensor or 'first' init; for 'k-means++' the same seed gives
        the same result on the same machine."""
        from . import cluster as _cluster
        G, max_iter = _cluster.check_args("kmeans", n_clusters, max_iter, init)
        pts = self._knn_rows("kmeans", "points", points)
        if isinstance(init, torch.Tensor):
            _cluster.check_init_tensor("kmeans", init, G, pts)
        if pts.shape[0] > 2 ** 31 - 64:
            raise ValueError(f"kmeans: {pts.shape[0]} points are beyond one call of the library")
        self._on_device("kmeans", "points", pts)
        pts = pts.contiguous()
        if isinstance(init, torch.Tensor):
            start = init
        elif init == "first":
            start = _cluster.init_first(pts, G)
        else:
            start = _cluster.init_plus_plus(pts, G, seed)
        return _cluster.lloyd(self._handle(), pts, start, max_iter)

    def silhouette(self, points, labels, n_clusters=None, metric="euclidean"):
        """The exact silhouette of the rows of ``points`` [N, Kx] under ``labels``: per row its mean distance to
        the other rows of its cluster (a), the smallest mean distance to the rows of another cluster (b, that
        cluster in 'nearest') and s = (b - a) / max(a, b); per cluster the mean of s; and their overall mean, the
        score that answers "how many clusters?" where ``kmeans``' inertia only falls.  One library call
        (include/spmf_hip.h spmf_silhouette has the definition, csrc/silhouette.hip): every pair of rows on the
        matrix cores, fp64 sums in a fixed order, no [N, N] or [N, G] array.

        ``points``: a float32 tensor on the model's device with 1 <= Kx <= 256 whatever the model's latent_dim.
        ``labels``: 1-D integers (numpy or torch on any device), one per row, in {-1, 0 .. n_clusters - 1}; -1 is
        "no cluster" (what ``kmeans`` gives a non-finite row).  ``n_clusters`` (at most 65536) defaults to
        max(labels) + 1.  ``metric``: 'euclidean' or 'cosine' (the distance 1 - cos).  A row with label -1 or a
        non-finite value (under 'cosine' a zero row too) is no member of any cluster: its outputs are NaN /
        nearest -1 and it changes no bit of any other row's result.

        Returns device tensors 'silhouette', 'a', 'b' (float32 [N]), 'nearest' (int32 [N]), 'cluster_mean'
        (fp64 [G], NaN for an empty cluster) and 'counts' (int64 [G], the members), and the host values 'score'
        (the sum of the clusters' fp64 sums of s over the number of members; NaN with fewer than two non-empty
        clusters) and 'n_scored' (the members).  A singleton cluster's row has s = 0.  Bit-reproducible.

        Cost and accuracy: N^2 pairs -- sample rows (``points[idx]``, ``labels[idx]``) where that is too many.
        Distances come from the fp32 expansion |x_i|^2 + |x_j|^2 - 2 <x_i, x_j> of centred (or unit) rows: the
        absolute error of one squared distance is about 2^-24 * KP * (|x'_i|^2 + |x'_j|^2), with KP the width
        rounded up to 4, 8, .., 256, so distances far below the rows' norms are coarse.  Separated clusters are
        scored to fp32 accuracy; a near-collinear cloud with large norms (an untrained model's embedding) is
        scored coarsely."""
        from . import neighbors as _neighbors
        pts = self._knn_rows("silhouette", "points", points)
        if metric not in _neighbors.METRICS:
            raise ValueError(f"silhouette: metric must be one of {_neighbors.METRICS}, got {metric!r}")
        if n_clusters is not None:
            _args.integer("silhouette", "n_clusters", n_clusters)
        labels = _vector("silhouette", "labels", labels)
        N, width = int(pts.shape[0]), int(pts.shape[1])
        if int(labels.numel()) != N:
            raise ValueError(f"silhouette: labels must have one entry per row, got {int(labels.numel())} for "
                             f"{N} rows")
        G = self._label_range("silhouette", labels, n_clusters, "n_clusters")
        if G > 65536:
            raise ValueError(f"silhouette: n_clusters must be at most 65536, got {G}")
        if N > 2 ** 31 - 64:
            raise ValueError(f"silhouette: {N} points are beyond one call of the library")
        self._on_device("silhouette", "points", pts)
        pts = pts.contiguous()
        labels = labels.to(device=pts.device, dtype=torch.int32).contiguous()
        sil, a, b = (torch.empty(N, dtype=torch.float32, device=pts.device) for _ in range(3))
        nearest = torch.empty(N, dtype=torch.int32, device=pts.device)
        sums = torch.empty(G, dtype=torch.float64, device=pts.device)
        counts = torch.empty(G, dtype=torch.int64, device=pts.device)
        _lib.call(self._handle(), "spmf_silhouette", pts.data_ptr(), N, width, labels.data_ptr(), G,
                  1 if metric == "cosine" else 0, sil.data_ptr(), a.data_ptr(), b.data_ptr(), nearest.data_ptr(),
                  sums.data_ptr(), counts.data_ptr(), device=pts.device,
                  scratch=(_lib.Scratch(pts.device), "spmf_silhouette_scratch_bytes", N, G, width))
        n = counts.to(torch.float64)
        mean = sums / n.masked_fill(counts == 0, float("nan"))
        total, members, nonempty = torch.stack([sums.sum(), n.sum(), (counts > 0).sum().to(torch.float64)]).tolist()
        score = total / members if nonempty >= 2 else float("nan")
        return {"silhouette": sil, "a": a, "b": b, "nearest": nearest, "cluster_mean": mean, "counts": counts,
                "score": score, "n_scored": int(members)}

    def fuzzy_graph(self, indices, distances):
        """The symmetric fuzzy neighbour graph of a ``knn`` result (``knn(points)`` on one set of rows): UMAP's
        graph, scanpy's ``obsp["connectivities"]``.  ``spmf_amd.graph.fuzzy_graph`` has the definition; plain
        torch in fp64 on the tensors' device, one stable sort and no scatter-add, so reproducible.  Returns
        {'indptr': int64 [N+1], 'indices': int32, 'weights': float32, 'sigma', 'rho': fp64 [N]}: what
        ``graph_layout`` takes, and ``spmf_amd.graph.to_csr`` turns it into the numpy CSR arrays."""
        from . import graph as _graph
        return _graph.fuzzy_graph(indices, distances)

    @staticmethod
    def _layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion, learning_rate,
                     seed, init, starts=None):
        """The layout arguments of ``graph_layout`` / ``umap`` / ``graph_transform`` that need no graph, checked
        before any library call -> namespace(n_epochs (or None), a, b, M, rate, gamma, lr, seed).  ``starts``: the
        values of ``init`` beside a tensor (default: ``spmf_amd.graph.INITS``)."""
        from . import graph as _graph

        def weight(what, v, positive=False):          # (a finite fp32)
            return _args.number(name, what, v, positive, hi=3.0e38)
        if n_epochs is not None:
            n_epochs = _args.integer(name, "n_epochs", n_epochs, 0, 2 ** 31 - 1)
        M = _args.integer(name, "n_negatives", n_negatives, 1, _graph.MAX_NEGATIVES)
        seed = _args.integer(name, "seed", seed, 0, 2 ** 64 - 1)
        rate, gamma = weight("negative_rate", negative_rate), weight("repulsion", repulsion)
        lr = weight("learning_rate", learning_rate)
        if (a is None) != (b is None):
            raise ValueError(f"{name}: a and b go together (both, or neither for the fit to min_dist and spread)")
        if a is None:
            try:
                a, b = _graph.find_ab(min_dist, spread)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{name}: {e}") from None
        else:
            a, b = weight("a", a, positive=True), weight("b", b, positive=True)
        starts = _graph.INITS if starts is None else starts
        if not isinstance(init, torch.Tensor) and not (isinstance(init, (str, type(None))) and init in starts):
            raise ValueError(f"{name}: init must be one of {starts} or a float32 [N, 2] tensor, got {init!r}")
        return SimpleNamespace(n_epochs=n_epochs, a=a, b=b, M=M, rate=rate, gamma=gamma, lr=lr, seed=seed)

    @staticmethod
    def _graph_tensors(name, graph):
        """The graph dict of ``graph_layout`` / ``spectral``, its types and shapes checked -> (indptr, indices,
        weights, N, nnz)."""
        if not isinstance(graph, dict) or any(n not in graph for n in ("indptr", "indices", "weights")):
            raise ValueError(f"{name}: graph must be a dict with 'indptr', 'indices' and 'weights' (fuzzy_graph)")
        want = {"indptr": torch.int64, "indices": torch.int32, "weights": torch.float32}
        for n, dt in want.items():
            t = graph[n]
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dt:
                raise ValueError(f"{name}: graph['{n}'] must be a 1-D {dt} tensor")
        indptr, indices, weights = (graph[n] for n in want)
        if indptr.numel() < 1:
            raise ValueError(f"{name}: graph['indptr'] must have N + 1 entries")
        N, nnz = int(indptr.numel()) - 1, int(indices.numel())
        if int(weights.numel()) != nnz:
            raise ValueError(f"{name}: graph['weights'] has {int(weights.numel())} entries, graph['indices'] {nnz}")
        if N > 2 ** 31 - 64:
            raise ValueError(f"{name}: {N} rows are beyond one call of the library")
        if indices.device != indptr.device or weights.device != indptr.device:
            raise ValueError(f"{name}: the graph's tensors must be on one device")
        return indptr, indices, weights, N, nnz

    @staticmethod
    def _graph_numbers(name, indptr, indices, N, nnz):
        """The graph's numbers -- an indptr rising from 0 to nnz, indices in [0, N) -- checked before any library
        call: one device-side reduction and one read-back."""
        ends = torch.stack([indptr[0], indptr[-1]])
        step = torch.diff(indptr).amin().reshape(1) if N else torch.zeros(1, dtype=torch.int64, device=indptr.device)
        span = torch.stack(list(torch.aminmax(indices))).to(torch.int64) if nnz else \
            torch.zeros(2, dtype=torch.int64, device=indptr.device)
        first, last, step, lo, hi = torch.cat([ends, step, span]).tolist()
        if first != 0 or last != nnz or step < 0:
            raise ValueError(f"{name}: graph['indptr'] must rise from 0 to the {nnz} entries, got {first} .. {last}"
                             + (" with a falling step" if step < 0 else ""))
        if nnz and (lo < 0 or hi >= N):
            raise ValueError(f"{name}: graph['indices'] must lie in [0, {N}), got {lo} .. {hi}")

    def graph_layout(self, graph, init="pca", points=None, n_epochs=None, min_dist=0.1, spread=1.0, a=None, b=None,
                     n_negatives=8, negative_rate=5.0, repulsion=1.0, learning_rate=1.0, seed=0):
        """A deterministic 2-D layout of a weighted graph: the full-batch form of UMAP's objective, one kernel
        launch per epoch (include/spmf_hip.h spmf_graph_layout has the definition, csrc/graph_layout.hip).  Every
        epoch moves every row at once from the positions of the epoch before: along its edges towards its
        neighbours, weighted by the edge, and away from ``n_negatives`` rows drawn by a counter-based generator
        from (``seed``, row, epoch); the step is divided by max(1, the row's summed weight), which keeps the
        simultaneous update from overshooting.  No atomics: two runs give the same bits.

        ``graph``: what ``fuzzy_graph`` returns -- 'indptr' int64 [N+1] (monotone from 0 to nnz), 'indices' int32
        in [0, N), 'weights' float32, on the model's device.  ``init``: a float32 [N, 2] tensor on the device;
        'pca': the two leading principal axes of ``points`` [N, Kx] (``spmf_amd.graph.init_pca``: fp64 covariance
        of the finite rows, max |coordinate| = 10, a non-finite row starts NaN and stays); 'random': uniform
        [-10, 10] from a CPU generator seeded with ``seed``.  ``n_epochs``: None is 500 for N <= 10 000, else 200.
        (``a``, ``b``): the curve 1 / (1 + a d^(2b)); None fits them to (``min_dist``, ``spread``) as umap-learn
        does.  ``negative_rate``: negatives per visit of an edge (umap-learn's negative_sample_rate), spread over
        the ``n_negatives`` (1..64) draws of a row; ``repulsion``: their strength; ``learning_rate``: the first
        epoch's step, falling linearly to 0.

        Returns {'embedding': float32 [N, 2] on the device, 'a', 'b', 'n_epochs'}.  Bit-reproducible for a tensor or
        'pca' init on one machine; for 'random' the same seed gives the same result."""
        from . import graph as _graph
        name = "graph_layout"
        la = self._layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                               learning_rate, seed, init)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        if isinstance(init, torch.Tensor):
            if init.dim() != 2 or tuple(init.shape) != (N, 2) or init.dtype != torch.float32:
                raise ValueError(f"{name}: an init tensor must be float32 of shape {(N, 2)}, got {init.dtype} "
                                 f"{tuple(init.shape)}")
            if init.device != indptr.device:
                raise ValueError(f"{name}: an init tensor must be on the device of the graph {indptr.device}, got "
                                 f"{init.device}")
        elif init == "pca":
            if not isinstance(points, torch.Tensor) or points.dim() != 2 or not points.dtype.is_floating_point \
                    or int(points.shape[0]) != N or int(points.shape[1]) < 1:
                raise ValueError(f"{name}: init='pca' needs points, a floating-point [N, Kx] tensor with N = {N} rows")
            if points.device != indptr.device:
                raise ValueError(f"{name}: points must be on the device of the graph {indptr.device}, got "
                                 f"{points.device}")
        self._graph_numbers(name, indptr, indices, N, nnz)
        self._on_device(name, "the graph", indptr)
        total = _graph.default_epochs(N) if la.n_epochs is None else la.n_epochs
        if isinstance(init, torch.Tensor):
            start = init.contiguous()
        elif init == "pca":
            start = _graph.init_pca(points)
        else:
            start = _graph.init_random(N, la.seed, indptr.device)
        indptr, indices, weights = indptr.contiguous(), indices.contiguous(), weights.contiguous()
        out = torch.empty(N, 2, dtype=torch.float32, device=indptr.device)
        _lib.call(self._handle(), "spmf_graph_layout", N, nnz, indptr.data_ptr(), indices.data_ptr(),
                  weights.data_ptr(), start.data_ptr(), out.data_ptr(), 0, total, total, la.lr, la.a, la.b, la.gamma,
                  la.rate, la.M, la.seed, device=indptr.device,
                  scratch=(_lib.Scratch(indptr.device), "spmf_graph_layout_scratch_bytes", N))
        return {"embedding": out, "a": la.a, "b": la.b, "n_epochs": total}

    def umap(self, data, k=15, metric="euclidean", nsamples=32, draws=None, max_rows=None, init="pca", n_epochs=None,
             min_dist=0.1, spread=1.0, a=None, b=None, n_negatives=8, negative_rate=5.0, repulsion=1.0,
             learning_rate=1.0, seed=0):
        """The 2-D map of the rows of ``data``: ``embed`` on ``data``, ``knn`` on the posterior mean encodings,
        ``fuzzy_graph`` on their result and ``graph_layout`` on the graph ('pca' starts from the encodings) --
        the coordinates scanpy keeps in ``obsm["X_umap"]``, on which clusters, factor scores and genes are looked
        at.  ``data``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed`` (the rows of all batches are
        concatenated); ``k`` and ``metric`` as in ``knn``; the layout arguments as in ``graph_layout`` (``init``: a
        tensor, 'pca' or 'random').

        Returns what ``graph_layout`` returns, bit for bit the four calls made by hand, and 'graph' (the fuzzy
        graph), 'latent' (the encoding, float32 [N, latent_dim]) and the 'indices' / 'distances' of ``knn``.
        Bit-reproducible for given draws with a tensor or 'pca' init on one machine; for 'random' the same seed
        gives the same result."""
        self._knn_args("umap", k, metric)
        self._layout_args("umap", n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                          learning_rate, seed, init)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"umap: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        nn = self.knn(emb, k=k, metric=metric)
        g = self.fuzzy_graph(nn["indices"], nn["distances"])
        res = self.graph_layout(g, init=init, points=emb, n_epochs=n_epochs, min_dist=min_dist, spread=spread, a=a,
                                b=b, n_negatives=n_negatives, negative_rate=negative_rate, repulsion=repulsion,
                                learning_rate=learning_rate, seed=seed)
        res.update(graph=g, latent=emb, indices=nn["indices"], distances=nn["distances"])
        return res

    def spectral(self, graph, n_components=2, tol=1e-4, max_iter=100, seed=0):
        """The ``n_components`` + 1 leading eigenvectors of S = D^-1/2 A D^-1/2 of a weighted graph: the spectral
        embedding of its rows (sklearn's ``SpectralEmbedding``, the start of umap-learn's layout, with
        ``spmf_amd.spectral.diffusion_map`` scanpy's ``tl.diffmap``).  Chebyshev-filtered subspace iteration on a
        block of 16 columns (``spmf_amd.spectral`` has the algorithm): the products with the graph and the two
        small fp64 reductions are the library's (include/spmf_hip.h spmf_graph_spmm, csrc/spectral.hip), the
        16 x 16 eigenproblems are ``eigh`` on the CPU.  No atomics and a seeded CPU start: two runs give the same
        bits.

        ``graph``: as in ``graph_layout``, what ``fuzzy_graph`` returns; it should be symmetric (an asymmetric one
        is not refused, it does not converge).  1 <= ``n_components`` <= 12.  The iteration stops when
        |S v - l v| <= ``tol`` for the n_components + 1 leading columns, or after ``max_iter`` outer iterations.
        At least 32 rows must have a valid edge: below that a dense ``eigh`` is the tool.

        Returns what ``spmf_amd.spectral.solve`` returns, tensors on the device: 'values', 'vectors', 'embedding'
        (``vectors[:, 1:]``), 'residuals', 'converged', 'n_iter', 'n_products', 'scale', 'n_unit'.  In a degenerate
        eigenspace the basis is whatever the seeded start gives: reproducible, not canonical.  Pass
        ``spmf_amd.spectral.layout_init(res['embedding'], seed)`` as ``graph_layout(init=...)`` for the spectral
        start of a layout."""
        from . import spectral as _spectral
        name = "spectral"
        _spectral.check_args(name, n_components, tol, max_iter, seed)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        self._graph_numbers(name, indptr, indices, N, nnz)
        # the rows with a valid edge, in plain torch: the library is not needed to refuse a small graph
        ok = (torch.isfinite(weights) & (weights > 0)).to(torch.int64)
        run = torch.cat([torch.zeros(1, dtype=torch.int64, device=ok.device), torch.cumsum(ok, 0)])
        n_live = int(((run[indptr[1:]] - run[indptr[:-1]]) > 0).sum())
        if n_live < _spectral.MIN_ROWS:
            raise _spectral.too_few_rows(name, n_live)
        self._on_device(name, "the graph", indptr)
        ops = _spectral.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _spectral.solve(ops, n_components, tol, max_iter, seed, name=name)

    def spectral_cluster(self, graph, n_clusters, tol=1e-4, max_iter=100, seed=0, kmeans_init="k-means++",
                         kmeans_max_iter=100):
        """Spectral clustering of the rows of a graph (Ng, Jordan, Weiss): ``spectral(n_components =
        n_clusters - 1)``, the rows of the ``n_clusters`` leading eigenvectors scaled to unit length
        (``spmf_amd.spectral.cluster_features``), then ``kmeans`` of those rows.  It separates clusters that are
        not convex in the latent space -- two concentric rings -- where ``cluster``'s k-means of the points
        cannot.  2 <= ``n_clusters`` <= 13; a row without a valid edge gets the label -1.

        Returns what ``kmeans`` returns (for the features) and 'spectral' (the result of ``spectral``) and
        'features'.  Bit-reproducible for a given seed on one machine."""
        from . import cluster as _cluster
        from . import spectral as _spectral
        name = "spectral_cluster"
        _args.integer(name, "n_clusters", n_clusters, 2, _spectral.MAX_COMPONENTS + 1)
        _spectral.check_args(name, int(n_clusters) - 1, tol, max_iter, seed)
        _cluster.check_args(name, int(n_clusters), kmeans_max_iter, kmeans_init)
        res = self.spectral(graph, n_components=int(n_clusters) - 1, tol=tol, max_iter=max_iter, seed=seed)
        feats = _spectral.cluster_features(res, int(n_clusters))
        out = self.kmeans(feats, int(n_clusters), init=kmeans_init, max_iter=kmeans_max_iter, seed=seed)
        out.update(spectral=res, features=feats)
        return out

    def communities(self, graph, resolution=1.0, max_levels=32, max_sweeps=100, tol=1e-7):
        """Louvain clustering of the rows of a weighted graph by modularity (scanpy's ``tl.louvain`` /
        ``tl.leiden`` on ``obsp["connectivities"]``): it finds the number of clusters itself, where ``cluster`` and
        ``spectral_cluster`` are told it.  ``spmf_amd.communities`` has the algorithm: the weights become int64
        fixed point (rint(w 2^24)), so every sum is exact in any order; a level is a run of synchronous sweeps, each
        one library call (include/spmf_hip.h spmf_graph_move, csrc/graph_move.hip) that moves every row at once from
        the labels of the sweep before, upwards in label on even sweeps and downwards on odd ones; between levels the
        communities become the rows of a coarser graph.  No atomics on floats anywhere: two runs give the same
        bits, which are also the bits of the numpy backend (``spmf_amd.communities.NumpyOps``).

        ``graph``: as in ``graph_layout``, what ``fuzzy_graph`` returns; it should be symmetric (an asymmetric one
        is not refused).  ``resolution`` > 0: the gamma of Q = in / M2 - gamma sum_c (tot_c / M2)^2, larger for
        more and smaller communities.  A level keeps its best labelling (Q above the best so far by more than
        ``tol``) and ends after an up and a down sweep that moved nothing, 4 sweeps without a new best or
        ``max_sweeps``; the levels end when one merged nothing, or after ``max_levels``.

        Returns what ``spmf_amd.communities.solve`` returns, tensors on the device: 'labels' int64 [N], communities
        numbered by descending size (ties by smallest member row), -1 for a row without a valid entry -- what
        ``group_means``, ``silhouette`` and ``neighbors.vote`` take; 'n_communities', 'sizes', 'modularity',
        'levels' (per level 'n_nodes', 'n_communities', 'modularity', 'n_sweeps', 'hit_max_sweeps') and
        'resolution'."""
        from . import communities as _communities
        name = "communities"
        _communities.check_args(name, resolution, max_levels, max_sweeps, tol)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        self._graph_numbers(name, indptr, indices, N, nnz)
        self._on_device(name, "the graph", indptr)
        ops = _communities.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _communities.solve(ops, resolution, max_levels, max_sweeps, tol, name=name)

    def geodesic(self, graph, sources, predecessors=False, max_sweeps=None):
        """Exact shortest-path distances along a graph of edge lengths from ``sources``: how far along the neighbour
        graph every row is from a root -- the base of pseudotime, Isomap-style landmark distances, the distance to
        the nearest row of a set.  ``spmf_amd.geodesic`` has the definition: synchronous relaxation in pull form,
        16 sources to a block, one library launch per sweep (include/spmf_hip.h spmf_graph_relax,
        csrc/graph_paths.hip: ``spmf_graph_spmm``'s access pattern in the (min, +) semiring, no atomic), repeated
        until a sweep changes nothing.  The fixed point is unique, so two runs give the same bits, which are also
        the bits of the numpy backend (``spmf_amd.geodesic.NumpyOps``) and of a float32 Dijkstra.

        ``graph``: as in ``graph_layout``, but 'weights' are LENGTHS: ``spmf_amd.geodesic.length_graph`` of a
        ``knn`` result, or ``spmf_amd.geodesic.lengths_from_weights`` of a ``fuzzy_graph``; an entry counts with a
        finite length > 0.  ``sources``: a 1-D integer tensor of row numbers, one column each, or a list of such
        tensors, one column per set (the distance to the nearest row of the set).  ``max_sweeps`` defaults to N;
        reaching it is reported through 'converged'.

        Returns what ``spmf_amd.geodesic.solve`` returns, tensors on the graph's device: 'distances' float32
        [N, S] (+inf: unreached), 'predecessors' int32 [N, S] (with ``predecessors``; ``spmf_amd.geodesic.path``
        walks them) or None, 'n_sweeps' and 'converged'.  A model on the CPU runs the numpy backend on a graph on
        the CPU; a model on a device takes the graph on that device only."""
        from . import geodesic as _geodesic
        name = "geodesic"
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        _geodesic.source_sets(name, sources, N)
        if max_sweeps is not None:
            _args.integer(name, "max_sweeps", max_sweeps, 1, 2 ** 31 - 1)
        self._graph_numbers(name, indptr, indices, N, nnz)
        if torch.device(self.device).type == "cpu":
            if indptr.device.type != "cpu":
                raise ValueError(f"{name}: the graph must be on the model's device {self.device}, got "
                                 f"{indptr.device}")
            ops = _geodesic.NumpyOps({"indptr": indptr, "indices": indices, "weights": weights})
        else:
            self._on_device(name, "the graph", indptr)
            ops = _geodesic.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _geodesic.solve(ops, sources, predecessors=bool(predecessors), max_sweeps=max_sweeps, name=name)

    def pseudotime(self, data, root, k=15, metric="euclidean", nsamples=32, draws=None, max_rows=None):
        """The pseudotime of the rows of ``data`` from ``root``: ``embed`` on ``data``, ``knn`` on the posterior mean
        encodings, ``spmf_amd.geodesic.length_graph`` of their result, ``geodesic`` from the root and
        ``spmf_amd.geodesic.pseudotime``: the distance along the neighbour graph divided by the largest finite one
        (dpt's convention: values in [0, 1], NaN for rows the root does not reach).  ``root``: a row number, or a
        1-D integer tensor of them, one column each.  ``data``, ``nsamples`` / ``draws`` and ``max_rows`` as in
        ``embed`` (the rows of all batches are concatenated); ``k`` and ``metric`` as in ``knn``.

        Returns {'pseudotime': float32 [N] (a row number) or [N, S] (a tensor), 'geodesic': float32 of that shape,
        the distances, 'n_sweeps', 'converged', 'graph' (the graph of lengths), 'latent' (the encoding, float32
        [N, latent_dim]) and the 'indices' / 'distances' of ``knn``} on the device, bit for bit the calls made by
        hand.  Bit-reproducible for given draws.  Needs a model on a device: ``embed`` and ``knn`` are the
        library's; on a CPU model the parts that have a numpy backend are called by hand (``geodesic`` on a graph of
        ``spmf_amd.geodesic.length_graph``, then ``spmf_amd.geodesic.pseudotime``)."""
        from . import geodesic as _geodesic
        name = "pseudotime"
        self._knn_args(name, k, metric)
        single = isinstance(root, (int, np.integer)) and not isinstance(root, bool)
        if not single and not isinstance(root, torch.Tensor):
            raise ValueError(f"{name}: root must be a row number or a 1-D integer tensor of them, got "
                             f"{type(root).__name__}")
        roots = torch.tensor([int(root)], dtype=torch.int64) if single else root
        _geodesic.source_sets(name, roots, 2 ** 63 - 1)          # the type and the sign; the range needs the rows
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"{name}: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        _geodesic.source_sets(name, roots, int(emb.shape[0]))
        nn = self.knn(emb, k=k, metric=metric)
        g = _geodesic.length_graph(nn["indices"], nn["distances"])
        res = self.geodesic(g, roots)
        dist = res["distances"][:, 0].contiguous() if single else res["distances"]
        return {"pseudotime": _geodesic.pseudotime(dist), "geodesic": dist, "n_sweeps": res["n_sweeps"],
                "converged": res["converged"], "graph": g, "latent": emb, "indices": nn["indices"],
                "distances": nn["distances"]}

    def _paga_args(self, name, graph, labels, n_groups):
        """The graph and the labels of ``paga`` / ``paga_init``, checked before any library load -> (indptr,
        indices, weights, labels as a 1-D integer tensor)."""
        from . import paga as _paga
        labels = _vector(name, "labels", labels)
        _paga.group_count(name, labels, n_groups)
        indptr, indices, weights, N, nnz = self._graph_tensors(name, graph)
        if int(labels.numel()) != N:
            raise ValueError(f"{name}: labels must have one entry per row, got {int(labels.numel())} for {N} rows")
        self._graph_numbers(name, indptr, indices, N, nnz)
        self._on_device(name, "the graph", indptr)
        return indptr, indices, weights, labels

    def paga(self, graph, labels, n_groups=None):
        """The coarse graph of the groups of a labelled graph (scanpy's ``tl.paga``): which groups touch in the
        neighbour graph, and how much more than if every row's entries were spread over all other rows alike.
        ``spmf_amd.paga`` has the definition: the weights become int64 fixed point, the entries are summed by
        (label of row, label of column) into dense G x G tables in one library call (include/spmf_hip.h
        spmf_graph_group_edges, csrc/graph_groups.hip) with integer atomics only, and one fp64 host function turns
        the integers into connectivities.  Two runs give the same bits, which are also the bits of the numpy
        backend (``spmf_amd.paga.NumpyOps``).

        ``graph``: as in ``graph_layout``, what ``fuzzy_graph`` returns, or ``spmf_amd.paga.knn_graph`` of a ``knn``
        result without padding.  ``labels``: 1-D integers (numpy or torch on any device), one per row, what
        ``communities``, ``cluster`` or ``spectral_cluster`` return; negative is "no group".  ``n_groups`` (at
        most 1024) defaults to max(labels) + 1.

        Returns what ``spmf_amd.paga.solve`` returns, tensors on the device: 'connectivities',
        'connectivities_tree' (its maximum spanning forest), 'expected' (fp64 [G, G]), 'edge_count', 'edge_weight'
        (int64 [G, G]), 'sizes' (int64 [G]) and 'n_groups'."""
        from . import paga as _paga
        name = "paga"
        indptr, indices, weights, labels = self._paga_args(name, graph, labels, n_groups)
        ops = _paga.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        return _paga.solve(ops, labels, n_groups, name=name)

    def paga_init(self, graph, labels, n_groups=None, seed=0, threshold=0.0, n_epochs=None, min_dist=0.1, spread=1.0,
                  a=None, b=None, n_negatives=8, negative_rate=5.0, repulsion=1.0, learning_rate=1.0):
        """The PAGA start of a layout (scanpy's ``tl.umap(init_pos='paga')``): ``paga``, then ``graph_layout`` of
        the coarse graph of the entries with connectivity > ``threshold`` from ``spmf_amd.paga.group_start`` (the
        groups on a circle), then ``spmf_amd.paga.layout_init``: every row starts in the box half way from its
        group's position to the group's strongest neighbour.  The layout arguments are ``graph_layout``'s, for the
        coarse graph; ``seed`` draws its negatives and the rows' places in their boxes.

        Returns {'init': float32 [N, 2] on the device, 'positions': float32 [G, 2], 'paga': the result of
        ``paga``}.  ``graph_layout(graph, init=res['init'])`` is then the PAGA-initialised map, which keeps the
        groups' global arrangement.  Bit-reproducible for a given seed on one machine."""
        from . import paga as _paga
        name = "paga_init"
        la = self._layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                               learning_rate, seed, "random")
        threshold = _args.number(name, "threshold", threshold)
        _args.integer(name, "seed", seed, 0, 2 ** 63 - 1)
        indptr, indices, weights, labels = self._paga_args(name, graph, labels, n_groups)
        ops = _paga.LibraryOps(_lib.load(), self._handle(), indptr, indices, weights)
        res = _paga.solve(ops, labels, n_groups, name=name)
        conn = res["connectivities"]
        coarse = _paga.coarse_graph(conn, threshold)
        start = _paga.group_start(res["n_groups"]).to(conn.device)
        lay = self.graph_layout(coarse, init=start, n_epochs=la.n_epochs, a=la.a, b=la.b, n_negatives=la.M,
                                negative_rate=la.rate, repulsion=la.gamma, learning_rate=la.lr, seed=la.seed)
        init = _paga.layout_init(labels, lay["embedding"], conn, seed=la.seed).to(conn.device)
        return {"init": init, "positions": lay["embedding"], "paga": res}

    def graph_transform(self, indices, distances, reference_layout, weights=None, init=None, n_epochs=None,
                        min_dist=0.1, spread=1.0, a=None, b=None, n_negatives=8, negative_rate=5.0, repulsion=1.0,
                        learning_rate=0.25, seed=0, row_offset=0):
        """New rows on a fitted layout, the reference rows held where they are (umap-learn's ``transform``): all
        epochs in one kernel launch (include/spmf_hip.h spmf_graph_transform has the definition,
        csrc/graph_transform.hip).  A new row starts at the weighted mean of its neighbours' positions and is
        then pulled towards them and pushed away from ``n_negatives`` reference rows drawn per epoch from
        (``seed``, the row's number, epoch).  A row's position is a function of that row alone: rows may be mapped
        in chunks of any size with the same bits, ``row_offset`` being the number of a chunk's first row.

        ``indices`` int [Q, k] and ``distances`` float [Q, k]: what ``knn(reference_points, queries=...)`` returned
        (k <= 64, padding -1 / +inf); ``reference_layout``: float32 [n_ref, 2], the 'embedding' of ``graph_layout``
        / ``umap``; all on the model's device.  ``weights``: float32 [Q, k] memberships, None for
        ``spmf_amd.graph.query_weights(indices, distances)``.  ``init``: None for the weighted mean, or a float32
        [Q, 2] tensor.  ``n_epochs``: None is umap-learn's rule for transform, 100 up to 10 000 rows, else 30.
        (``a``, ``b``) should be the reference layout's; None fits them to (``min_dist``, ``spread``).  The other
        arguments as in ``graph_layout``; the default ``learning_rate`` is a quarter of its, as in umap-learn.

        Returns {'embedding': float32 [Q, 2] on the device (NaN: a row without a valid neighbour), 'weights',
        'sigma' (None with given ``weights``), 'a', 'b', 'n_epochs'}.  Bit-reproducible."""
        from . import graph as _graph
        name = "graph_transform"
        la = self._layout_args(name, n_epochs, min_dist, spread, a, b, n_negatives, negative_rate, repulsion,
                               learning_rate, seed, init, starts=(None,))
        _args.integer(name, "row_offset", row_offset, 0)
        for what, t in (("indices", indices), ("distances", distances), ("reference_layout", reference_layout)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise ValueError(f"{name}: {what} must be a 2-D torch tensor")
        if indices.dtype.is_floating_point or indices.dtype == torch.bool:
            raise ValueError(f"{name}: indices must hold integers, got {indices.dtype}")
        if not distances.dtype.is_floating_point or distances.shape != indices.shape:
            raise ValueError(f"{name}: distances must be floating point of the shape of indices "
                             f"{tuple(indices.shape)}, got {distances.dtype} {tuple(distances.shape)}")
        Q, k = int(indices.shape[0]), int(indices.shape[1])
        if not 1 <= k <= 64:
            raise ValueError(f"{name} needs 1 <= k <= 64 neighbours per row, got {k}")
        if reference_layout.dtype != torch.float32 or int(reference_layout.shape[1]) != 2:
            raise ValueError(f"{name}: reference_layout must be float32 of shape [n_ref, 2], got "
                             f"{reference_layout.dtype} {tuple(reference_layout.shape)}")
        n_ref = int(reference_layout.shape[0])
        if n_ref > 2 ** 31 - 1:
            raise ValueError(f"{name}: {n_ref} reference rows are beyond the int32 index of a neighbour")
        if int(row_offset) + Q > 2 ** 32:
            raise ValueError(f"{name}: row_offset + the {Q} rows must stay within 2^32, got row_offset={row_offset}")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 \
                    or weights.shape != indices.shape:
                raise ValueError(f"{name}: weights must be a float32 tensor of shape {tuple(indices.shape)}")
        if isinstance(init, torch.Tensor) and (tuple(init.shape) != (Q, 2) or init.dtype != torch.float32):
            raise ValueError(f"{name}: an init tensor must be float32 of shape {(Q, 2)}, got {init.dtype} "
                             f"{tuple(init.shape)}")
        for what, t in (("indices", indices), ("distances", distances), ("reference_layout", reference_layout),
                        ("weights", weights), ("init", init)):
            if t is not None:
                self._on_device(name, what, t)
        total = _graph.default_transform_epochs(Q) if la.n_epochs is None else la.n_epochs
        sigma = None
        if weights is None:
            qw = _graph.query_weights(indices, distances)
            weights, sigma = qw["weights"], qw["sigma"]
        # (an index beyond int32 is no row of the reference: it stays outside [0, n_ref) through the cast)
        idx = indices.clamp(-1, n_ref).to(torch.int32).contiguous()
        w, ref = weights.contiguous(), reference_layout.contiguous()
        start = init.contiguous() if init is not None else None
        out = torch.empty(Q, 2, dtype=torch.float32, device=idx.device)
        _lib.call(self._handle(), "spmf_graph_transform", Q, k, idx.data_ptr(), w.data_ptr(), ref.data_ptr(), n_ref,
                  start.data_ptr() if start is not None else None, out.data_ptr(), int(row_offset), 0, total, total,
                  la.lr, la.a, la.b, la.gamma, la.rate, la.M, la.seed, device=idx.device)
        return {"embedding": out, "weights": weights, "sigma": sigma, "a": la.a, "b": la.b, "n_epochs": total}

    def umap_transform(self, data, reference, k=15, metric="euclidean", nsamples=32, draws=None, max_rows=None,
                       labels=None, n_classes=None, n_epochs=None, learning_rate=0.25, n_negatives=8,
                       negative_rate=5.0, repulsion=1.0, seed=0):
        """The rows of ``data`` on the map of ``reference`` (what ``umap`` returned: its 'latent', 'embedding', 'a'
        and 'b' are used): ``embed`` on ``data``, ``knn`` of the encodings among the reference's, then
        ``graph_transform`` with the reference's curve -- umap-learn's ``transform``, scanpy's ``ingest``.  The
        reference map does not move.  ``data``, ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed``; ``k``
        and ``metric`` as in ``knn``; the layout arguments as in ``graph_transform``.  ``labels``: an integer per
        reference row (-1: none), e.g. the labels of ``cluster``; every new row then gets the class with the
        largest summed membership among its neighbours (``spmf_amd.neighbors.vote``; ``n_classes`` as there).

        Returns what ``graph_transform`` returns, bit for bit the calls made by hand, and 'latent' (the encoding,
        float32 [Q, latent_dim]), the 'indices' / 'distances' of ``knn`` and, with ``labels``, 'labels' int64 [Q]
        (-1: no voting neighbour) and 'label_share' fp64 [Q].  Bit-reproducible for given draws."""
        from . import neighbors as _neighbors
        name = "umap_transform"
        self._knn_args(name, k, metric)
        if not isinstance(reference, dict) or any(n not in reference for n in ("latent", "embedding", "a", "b")):
            raise ValueError(f"{name}: reference must be what umap returned: a dict with 'latent', 'embedding', "
                             f"'a' and 'b'")
        self._layout_args(name, n_epochs, 0.1, 1.0, reference["a"], reference["b"], n_negatives, negative_rate,
                          repulsion, learning_rate, seed, None, starts=(None,))
        lat, ref = reference["latent"], reference["embedding"]
        if not isinstance(lat, torch.Tensor) or lat.dim() != 2 or lat.dtype != torch.float32 \
                or int(lat.shape[1]) != self.latent_dim:
            raise ValueError(f"{name}: reference['latent'] must be a float32 [n_ref, {self.latent_dim}] tensor")
        if not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 \
                or tuple(ref.shape) != (int(lat.shape[0]), 2):
            raise ValueError(f"{name}: reference['embedding'] must be a float32 {(int(lat.shape[0]), 2)} tensor")
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"{name}: latent_dim {self.latent_dim} is beyond the 256 columns of knn")
        if labels is not None:
            labels = _vector(name, "labels", labels)
            if int(labels.numel()) != int(lat.shape[0]):
                raise ValueError(f"{name}: labels must have one entry per reference row, got {int(labels.numel())} "
                                 f"for {int(lat.shape[0])} rows")
            if n_classes is not None:
                _args.integer(name, "n_classes", n_classes, 0)
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        nn = self.knn(lat, k=k, queries=emb, metric=metric)
        res = self.graph_transform(nn["indices"], nn["distances"], ref, n_epochs=n_epochs, a=reference["a"],
                                   b=reference["b"], n_negatives=n_negatives, negative_rate=negative_rate,
                                   repulsion=repulsion, learning_rate=learning_rate, seed=seed)
        res.update(latent=emb, indices=nn["indices"], distances=nn["distances"])
        if labels is not None:
            res["labels"], res["label_share"] = _neighbors.vote(nn["indices"], res["weights"],
                                                                labels.to(emb.device), n_classes)
        return res

    def cluster(self, data, n_clusters, nsamples=32, draws=None, max_rows=None, init="k-means++", max_iter=100,
                seed=0):
        """k-means of the rows of ``data`` in the model's latent space: ``embed`` on ``data``, then ``kmeans``
        on the posterior mean encodings, with no labelling leaving the device in between.  ``data``,
        ``nsamples`` / ``draws`` and ``max_rows`` as in ``embed`` (the rows of all batches are concatenated);
        ``n_clusters``, ``init``, ``max_iter`` and ``seed`` as in ``kmeans``.

        Returns what ``kmeans`` returns, bit for bit ``kmeans(embed(data, draws=draws)["mean"], ...)``, and
        'embedding': float32 [N, latent_dim].  The labels are those ``group_means`` takes, and
        ``silhouette(res["embedding"], res["labels"], n_clusters)`` scores the clustering."""
        from . import cluster as _cluster
        G, max_iter = _cluster.check_args("cluster", n_clusters, max_iter, init)
        if not 1 <= self.latent_dim <= 256:
            raise ValueError(f"cluster: latent_dim {self.latent_dim} is beyond the 256 columns of kmeans")
        if isinstance(init, torch.Tensor):        # (its device is checked against the embedding's, in kmeans)
            if init.dim() != 2 or tuple(init.shape) != (G, self.latent_dim):
                raise ValueError(f"cluster: an init tensor must have shape {(G, self.latent_dim)}, got "
                                 f"{tuple(init.shape)}")
            if init.dtype != torch.float32:
                raise ValueError(f"cluster: an init tensor must be float32, got {init.dtype}")
        emb = self.embed(data, nsamples=nsamples, draws=draws, max_rows=max_rows)["mean"]
        res = self.kmeans(emb, G, init=init, max_iter=max_iter, seed=seed)
        res["embedding"] = emb
        return res
