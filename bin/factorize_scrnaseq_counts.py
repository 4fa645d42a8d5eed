#!/usr/bin/env python3
"""Factorize a single-cell RNA-seq count matrix with the log-transform decoder
-- the numeric half of the reference's scRNA script
(bin/factorize_scrnaseq_counts.py:29-140), which is where BASELINE config C4's
model comes from: ``log_transform=True``, ``column_norms`` = plain gene means
(:60,93-99), ``u_tau_scale = 1/sqrt(D*N)``, ``calibrate_advi(num_steps=500,
learning_rate=0.01, abs_tol=1e-3, rel_tol=1e-3, clip_value=10)`` (:101-105).

The reference script hard-codes a dataset directory (:30-35) and draws figures
with matplotlib/scanpy (:142-293); here the paths are flags and the figures are
replaced by a text table of the top genes per factor (what the first figure
shows, :154-159).

Inputs
  --counts   <name>_counts.npy ([cells, genes] dense) or a scipy .npz CSR
  --genes    <name>_genenames.npy (optional)
Outputs next to --counts (reference :124-130), <stem> = the counts file minus
"_counts.npy":
  <stem>_U_<P>.npy  encoding matrix          <stem>_V_<P>.npy  decoding matrix
  <stem>_W_<P>.npy  intercept                <stem>_Z_<P>.npy  encode(X)
  <stem>_cellscore_<P>.npy       Z * row size factors        (:113-114)
  <stem>_genescore_<P>.npy       V * gene means              (:118-119)
  <stem>_interceptscore_<P>.npy  W * gene means              (:108-109)
With --labels FILE.npy (one integer per cell, -1 = no group; e.g. a clustering of the neighbour graph):
  <stem>_groupmean_<P>.npy       [groups, genes] posterior predictive mean expression per group
and, per group, the --top genes by log2 fold change against the rest (mean over the draws, with its sd and the
share of draws beyond one doubling).  Without the flag nothing changes.
With --clusters G (deterministic k-means of the cells in the latent space, on the device):
  <stem>_cluster_<P>.npy         [cells] int32: the cluster of every cell (-1: a cell without a finite encoding)
  <stem>_centroid_<P>.npy        [G, P] float32: the centroids in the latent space
over the mean encoding of --cluster-draws posterior draws, started by k-means++ with --cluster-seed (which also
seeds the draws).  Without --labels these labels feed the group table above; with --labels the file wins for
the table.  Without the flag nothing changes.
With --silhouette (beside --clusters or --labels; the clusters when both are given):
  <stem>_silhouette_<P>.npy      [cells] float32: the silhouette of every cell in the latent space under those
                                 labels (NaN: a cell without a label or a finite encoding)
over the mean encoding of --cluster-draws posterior draws seeded by --cluster-seed (the encoding --clusters
works on), and the overall score with the mean per cluster: all pairs of cells, exactly.
With --umap (the 2-D map on which cells, clusters and factor scores are looked at):
  <stem>_UMAP_<P>.npy            [cells, 2] float32: the layout of the cells' fuzzy neighbour graph in the latent
                                 space (NaN: a cell without a finite encoding) -- the file the reference's
                                 plotting script loads as <dataset>_UMAP_scanpy.npy
from --umap-neighbors neighbours per cell, --umap-min-dist and --umap-epochs (default: 500 up to 10 000 cells,
200 above), over the mean encoding of --cluster-draws posterior draws seeded by --cluster-seed (the encoding
--clusters labels; the seed also draws the layout's negatives).  Without the flag nothing changes.
--umap-init spectral starts the layout from the two leading non-trivial eigenvectors of the graph (umap-learn's
default start) in place of the encoding's principal axes (--umap-init pca, the default).
With --spectral N (the spectral embedding / diffusion-map coordinates of the cells, 1 <= N <= 12):
  <stem>_spectral_<P>.npy        [cells, N] float32: the eigenvectors 1 .. N of D^-1/2 A D^-1/2 of the same fuzzy
                                 neighbour graph (0: a cell without a neighbour)
  <stem>_spectral_values_<P>.npy [N + 1] float64: the eigenvalues 0 .. N, descending, the first about 1
over the same encoding, --umap-neighbors and seed.  Without the flag nothing changes.
With --communities (Louvain clustering of the same fuzzy neighbour graph by modularity: the number of clusters is
found, not given; --resolution R, default 1, larger for more and smaller communities):
  <stem>_communities_<P>.npy     [cells] int64: the community of every cell, numbered by descending size (-1: a
                                 cell without a neighbour)
over the same encoding, --umap-neighbors and seed; with --umap the graph is built once.  The labels stand in for
--clusters wherever those are used and --clusters is not given: the group table (without --labels), --silhouette
and the labels of --map-counts.  Bit-reproducible for a given model.  Without the flag nothing changes.
With --paga (the coarse graph of the clusters, scanpy's tl.paga, over the same fuzzy neighbour graph; the labels are
those of --communities, else of --clusters, else of --labels, and one of the three is needed):
  <stem>_paga_connectivities_<P>.npy  [groups, groups] float64: how much more than chance two groups touch, in [0, 1]
  <stem>_paga_tree_<P>.npy            [groups, groups] float64: the maximum spanning forest of the connectivities
  <stem>_paga_pos_<P>.npy             [groups, 2] float32: the layout of the coarse graph
--umap-init paga (which implies --paga) starts the layout of --umap from those positions, every cell in the box half
way from its group to the group's strongest neighbour (scanpy's init_pos='paga').  Without the flags nothing changes.
With --pseudotime ROOT (how far along the cells' neighbour graph every cell is from cell number ROOT: the exact
shortest-path distance over the symmetric graph of the same --umap-neighbors neighbours, their latent distances the
lengths, divided by the largest one; the ordering put next to --paga):
  <stem>_pseudotime_<P>.npy      [cells] float32 in [0, 1] (NaN: a cell the root does not reach)
  <stem>_paga_pseudotime_<P>.npy [groups] float64, with --paga: the mean pseudotime of every group's reached cells
                                 (NaN: a group without one)
over the same encoding and seed; the neighbours --umap, --communities or --paga found in the same run are used again.
Without the flag nothing changes.
With --map-counts FILE beside --umap (new cells over the same genes, e.g. a second sample; .npy dense or .npz CSR):
  <stem>_UMAP_map_<P>.npy        [new cells, 2] float32: the new cells on the map above, which does not move (NaN:
                                 a cell without a finite encoding)
  <stem>_label_map_<P>.npy       [new cells] int64, with --clusters or --labels: the label with the largest summed
                                 membership among a new cell's --umap-neighbors nearest cells of --counts (-1: none;
                                 the clusters when both are given)
over the same draws and seed.  Without the flag nothing changes.
With --gene-sets FILE.gmt (tab-separated: set name, description, member gene names, looked up in --genes):
  <stem>_setscore_<P>.npy        [cells, sets] posterior predictive expression summed over each gene set
  <stem>_setscore_sd_<P>.npy     [cells, sets] its standard deviation over the --set-draws posterior draws
Without the flag nothing changes.
With --gene-waic (model criticism per gene: which genes the model fits badly):
  <stem>_genewaic_<P>.npy        [genes, 6] float64: n, n_excluded, lppd, pwaic, waic, se of every gene's
                                 cells over the --waic-draws posterior draws, in gene order
and the --top genes with the largest waic per counted cell.  Without the flag nothing changes.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mederrata_spmf import PoissonMatrixFactorization  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Log-transform PMF of a scRNA-seq count matrix")
    p.add_argument("--counts", required=True, help="<name>_counts.npy or a scipy .npz CSR")
    p.add_argument("--genes", default=None, help="<name>_genenames.npy")
    p.add_argument("-d", "--dimension", type=int, default=3, help="latent factors P (reference: 3)")
    p.add_argument("-b", "--batch-size", type=int, default=256, help="reference: 256")
    p.add_argument("-e", "--epoch", type=int, default=500, help="num_steps (reference: 500)")
    p.add_argument("-lr", "--learning-rate", type=float, default=0.01)
    p.add_argument("-c", "--clip-value", type=float, default=10.0)
    p.add_argument("--abs-tol", type=float, default=1e-3)
    p.add_argument("--rel-tol", type=float, default=1e-3)
    p.add_argument("--top", type=int, default=10, help="genes listed per factor")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--labels", default=None, help="FILE.npy: a group per cell (-1: none); adds the group means "
                                                  "and the marker genes per group")
    p.add_argument("--group-draws", type=int, default=32, help="posterior draws of the group means")
    p.add_argument("--clusters", type=int, default=None, help="G: k-means of the cells in the latent space into G "
                                                              "clusters; writes the labels and the centroids")
    p.add_argument("--cluster-seed", type=int, default=0, help="seed of the k-means++ start and of the draws")
    p.add_argument("--cluster-draws", type=int, default=32, help="posterior draws of the clustered encoding")
    p.add_argument("--silhouette", action="store_true", help="with --clusters or --labels: the silhouette of "
                                                             "every cell under those labels, and the score")
    p.add_argument("--umap", action="store_true", help="writes the 2-D layout of the cells' neighbour graph in the "
                                                       "latent space")
    p.add_argument("--umap-neighbors", type=int, default=15, help="neighbours per cell of the layout's graph")
    p.add_argument("--umap-min-dist", type=float, default=0.1, help="min_dist of the layout's curve")
    p.add_argument("--umap-epochs", type=int, default=None, help="epochs of the layout (default: by size)")
    p.add_argument("--umap-init", choices=("pca", "spectral", "paga"), default="pca", help="the layout's start: the "
                   "encoding's principal axes, the graph's leading eigenvectors, or the layout of the groups' "
                   "coarse graph (implies --paga)")
    p.add_argument("--spectral", type=int, default=None, help="N: writes the N leading non-trivial eigenvectors "
                                                              "of the cells' neighbour graph and their eigenvalues")
    p.add_argument("--communities", action="store_true", help="writes the Louvain communities of the cells' neighbour "
                                                              "graph (the number of clusters is found)")
    p.add_argument("--resolution", type=float, default=1.0, help="R > 0: the resolution of --communities' modularity")
    p.add_argument("--paga", action="store_true", help="with --communities, --clusters or --labels: writes the "
                                                       "connectivities of those groups in the neighbour graph, "
                                                       "their spanning forest and the coarse graph's layout")
    p.add_argument("--pseudotime", type=int, default=None, metavar="ROOT", help="a cell number: writes every cell's "
                   "distance from that cell along the neighbour graph, scaled to [0, 1] (with --paga also the "
                   "groups' means)")
    p.add_argument("--map-counts", default=None, help="FILE: new cells over the same genes; with --umap they are "
                                                      "placed on the map (and labelled with --clusters / --labels)")
    p.add_argument("--gene-sets", default=None, help="FILE.gmt: gene sets (name, description, members per line); "
                                                     "adds a score per cell and set with its posterior sd")
    p.add_argument("--set-draws", type=int, default=32, help="posterior draws of the gene-set scores (>= 2)")
    p.add_argument("--gene-waic", action="store_true", help="adds the WAIC of every gene's cells (lppd, pwaic, "
                                                            "waic, se) and lists the worst-fitted genes")
    p.add_argument("--waic-draws", type=_at_least_two, default=32, help="posterior draws of the per-gene WAIC "
                                                                        "(>= 2)")
    return p


def _at_least_two(text):
    n = int(text)
    if n < 2:
        raise argparse.ArgumentTypeError("at least 2 draws (the variance over the draws needs two)")
    return n


def load_counts(path):
    if path.endswith(".npz"):
        import scipy.sparse as sp
        return sp.load_npz(path).tocsr()
    return np.load(path)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if args.silhouette and args.clusters is None and args.labels is None and not args.communities:
        parser.error("--silhouette needs --clusters, --communities or --labels")
    if args.umap_init == "paga":
        args.paga = True
    if args.paga and not args.communities and args.clusters is None and args.labels is None:
        parser.error("--paga needs --communities, --clusters or --labels")
    if not (args.resolution > 0 and args.resolution < float("inf")):
        parser.error("--resolution needs a finite R > 0")
    if args.map_counts is not None and not args.umap:
        parser.error("--map-counts needs --umap")
    if args.pseudotime is not None and args.pseudotime < 0:
        parser.error("--pseudotime needs a cell number >= 0")
    if args.spectral is not None and not 1 <= args.spectral <= 12:
        parser.error("--spectral needs 1 <= N <= 12")
    if args.map_counts is not None and not os.path.exists(args.map_counts):
        sys.exit("File doesn't exist")
    if not os.path.exists(args.counts):
        sys.exit("File doesn't exist")
    import torch
    if args.seed is not None:
        torch.manual_seed(args.seed)
    X = load_counts(args.counts)
    N, D = X.shape
    P, B = args.dimension, args.batch_size
    gene_names = (np.load(args.genes, allow_pickle=True) if args.genes
                  else np.array([f"g{j}" for j in range(D)], dtype=object))

    row_sums = np.asarray(X.sum(1)).reshape(-1).astype(np.float64)
    row_size_factors = row_sums / np.median(row_sums)                     # :48-50
    col_norm = np.asarray(X.mean(0)).reshape(-1).astype(np.float64)       # :56,60
    # (a gene with no counts would divide by zero in g(x) = log(x/eta + 1))
    col_norm = np.maximum(col_norm, 1e-3)

    print((N, D))
    print(f"Total observations={N}, Batch size={B}: dropping {N % B} observations.")   # :76-77
    nb = N // B
    if nb == 0:
        sys.exit("fewer cells than one batch")
    if args.pseudotime is not None and args.pseudotime >= N:
        sys.exit(f"--pseudotime must be one of the {N} cells, got {args.pseudotime}")
    # shuffle once, batch with drop_remainder (:86-87); the batches stay resident on the device
    perm = np.random.default_rng(args.seed).permutation(N)
    batches = []
    for i in range(nb):
        idx = np.sort(perm[i * B:(i + 1) * B])
        xb = X[idx]
        batches.append({"data": xb, "indices": idx, "normalization": row_size_factors[idx]})

    factor = PoissonMatrixFactorization(
        batches, latent_dim=P, strategy=None, scale_rates=True, column_norms=col_norm,
        log_transform=True, u_tau_scale=1.0 / np.sqrt(D * N), count_key="data")       # :91-99
    losses = factor.calibrate_advi(
        num_steps=args.epoch, learning_rate=args.learning_rate,
        abs_tol=args.abs_tol, rel_tol=args.rel_tol, clip_value=args.clip_value)        # :101-105

    U = factor.encoding_matrix().cpu().numpy()                                         # :111
    W = factor.intercept_matrix().cpu().numpy()                                        # :114
    intercept_score = W * col_norm[np.newaxis, :]
    Z = factor.encode(X).cpu().numpy()                                                 # :118
    cell_score = Z * row_size_factors[:, np.newaxis]
    V = factor.decoding_matrix().cpu().numpy()                                         # :122
    gene_score = V * col_norm[np.newaxis, :]

    stem = args.counts
    for suffix in ("_counts.npy", "_counts.npz", ".npy", ".npz"):
        if stem.endswith(suffix):
            stem = stem[:-len(suffix)]
            break
    for name, arr in (("U", U), ("V", V), ("W", W), ("Z", Z), ("cellscore", cell_score),
                      ("genescore", gene_score), ("interceptscore", intercept_score)):
        np.save(f"{stem}_{name}_{P}.npy", arr)                                         # :124-130

    # the first figure's content (:150-159): top genes per factor by gene score
    for p in range(P):
        top = np.argsort(gene_score[p, :])[::-1][:args.top]
        print(f"factor {p}: " + ", ".join(f"{gene_names[j]}({gene_score[p, j]:.3g})" for j in top))
    top = np.argsort(W[0, :])[::-1][:P * args.top]                                     # :174-175
    print("intercept: " + ", ".join(str(gene_names[j]) for j in top))
    clusters = None
    if args.clusters is not None:
        clusters = cluster_cells(factor, X, f"{stem}_cluster_{P}.npy", f"{stem}_centroid_{P}.npy", args)
    reference, n_clusters = None, args.clusters
    cells, paga_labels, paga_groups = None, None, None
    if args.paga or (args.pseudotime is not None and not args.umap):
        # the graph once, for the communities, the coarse graph, a layout that starts from it and the pseudotime
        cells = _cell_graph(factor, X, args)
    if args.paga:
        if clusters is not None:
            paga_labels, paga_groups = clusters, args.clusters
        elif args.labels is not None:
            paga_labels = np.load(args.labels)
    if args.communities:
        # the graph once: with --umap the layout comes first and its graph is clustered
        if args.umap and args.umap_init != "paga":
            reference = umap_cells(factor, X, f"{stem}_UMAP_{P}.npy", args)
        graph = reference["graph"] if reference is not None else cells[2] if cells is not None else None
        found, n_found = community_cells(factor, X, graph, f"{stem}_communities_{P}.npy", args)
        if clusters is None and n_found > 0:
            clusters, n_clusters = found, n_found
        if n_found > 0:
            paga_labels, paga_groups = found, n_found
    start = None
    if args.paga:
        start = paga_cells(factor, cells[2], paga_labels, paga_groups, f"{stem}_paga_connectivities_{P}.npy",
                           f"{stem}_paga_tree_{P}.npy", f"{stem}_paga_pos_{P}.npy", args)
    if args.labels is not None:
        group_table(factor, X, np.load(args.labels), gene_names, f"{stem}_groupmean_{P}.npy", args)
    elif clusters is not None:
        group_table(factor, X, clusters, gene_names, f"{stem}_groupmean_{P}.npy", args, n_groups=n_clusters)
    if args.silhouette:
        if clusters is not None:
            silhouette_cells(factor, X, clusters, n_clusters, f"{stem}_silhouette_{P}.npy", args)
        elif args.labels is not None:
            silhouette_cells(factor, X, np.load(args.labels), None, f"{stem}_silhouette_{P}.npy", args)
        else:
            print("silhouette: no cell has a community")
    if args.umap:
        if reference is None and args.umap_init == "paga":
            reference = umap_cells(factor, X, f"{stem}_UMAP_{P}.npy", args, start=(cells, start))
        elif reference is None:
            reference = umap_cells(factor, X, f"{stem}_UMAP_{P}.npy", args)
        if args.map_counts is not None:
            known = clusters if clusters is not None else (np.load(args.labels) if args.labels is not None else None)
            X_new = load_counts(args.map_counts)
            if X_new.ndim != 2 or X_new.shape[1] != D:
                sys.exit(f"--map-counts must hold [cells, {D}] counts over the genes of --counts, got {X_new.shape}")
            map_cells(factor, X_new, reference, known,
                      n_clusters if clusters is not None else None, f"{stem}_UMAP_map_{P}.npy",
                      f"{stem}_label_map_{P}.npy", args)
    if args.pseudotime is not None:
        # the neighbours of the run: the layout's, else those of the graph made above
        nn = reference if reference is not None else cells[1]
        pseudotime_cells(factor, nn, args.pseudotime, f"{stem}_pseudotime_{P}.npy",
                         paga_labels if args.paga else None, paga_groups, f"{stem}_paga_pseudotime_{P}.npy")
    if args.spectral is not None:
        spectral_cells(factor, X, f"{stem}_spectral_{P}.npy", f"{stem}_spectral_values_{P}.npy", args)
    if args.gene_sets is not None:
        gene_set_scores(factor, X, gene_names, f"{stem}_setscore_{P}.npy", f"{stem}_setscore_sd_{P}.npy", args)
    if args.gene_waic:
        gene_waic(factor, X, gene_names, f"{stem}_genewaic_{P}.npy", args)
    return losses


def gene_waic(factor, X, gene_names, path, args):
    """The per-gene WAIC: n, n_excluded, lppd, pwaic, waic and se of every gene's cells, and the genes with the
    largest waic per counted cell."""
    res = factor.waic_streaming({factor.count_key: X}, nsamples=args.waic_draws, col_scores=True)
    table = np.stack([res[k].cpu().numpy().astype(np.float64) for k in
                      ("col_n", "col_n_excluded", "col_lppd", "col_pwaic", "col_waic", "col_se")], axis=1)
    np.save(path, table)
    per_cell = np.where(table[:, 0] > 0, table[:, 4] / np.maximum(table[:, 0], 1.0), -np.inf)
    top = np.argsort(per_cell, kind="stable")[::-1][:args.top]
    print(f"gene waic: {res['waic']:.6g} over {res['n']} cells ({res['n_excluded']} excluded); worst per cell: "
          + ", ".join(f"{gene_names[j]}({per_cell[j]:.3g})" for j in top))


def gene_set_scores(factor, X, gene_names, path, sd_path, args):
    """The gene-set scores: per cell and set the posterior predictive expression summed over the set's genes
    and its standard deviation over the draws."""
    from spmf_amd import sets as gene_sets
    set_names, sets, dropped = gene_sets.read_gmt(args.gene_sets, gene_names)
    print(f"gene sets: {len(sets)} sets, {sum(len(s) for s in sets)} members, {dropped} unknown members dropped")
    res = factor.set_scores({factor.count_key: X}, sets, nsamples=args.set_draws, sd=True)
    np.save(path, res["mean"].cpu().numpy())
    np.save(sd_path, res["sd"].cpu().numpy())


def cluster_cells(factor, X, labels_path, centroid_path, args):
    """k-means of the cells in the latent space (``cluster``): the labels and the centroids as files; -> the
    labels on the device, as ``group_means`` takes them (only the files' copies leave it)."""
    import torch
    torch.manual_seed(args.cluster_seed)                  # the posterior draws of the encoding
    res = factor.cluster({factor.count_key: X}, args.clusters, nsamples=args.cluster_draws,
                         seed=args.cluster_seed)
    labels = res["labels"]
    np.save(labels_path, labels.cpu().numpy())
    np.save(centroid_path, res["centroids"].cpu().numpy())
    sizes = ", ".join(str(n) for n in res["counts"].tolist())
    print(f"clusters: {args.clusters} after {res['n_iter']} iterations"
          f"{'' if res['converged'] else ' (not converged)'}, inertia {res['inertia']:.6g}, cells {sizes}"
          + (f", {res['n_unassigned']} without a cluster" if res["n_unassigned"] else ""))
    return labels


def silhouette_cells(factor, X, labels, n_clusters, path, args):
    """The silhouette of the cells under ``labels`` in the latent space (``silhouette`` on the encoding that
    ``cluster_cells`` works on: the same seed, the same draws): the per-cell file, the score and the mean per
    cluster."""
    import torch
    torch.manual_seed(args.cluster_seed)                  # the posterior draws of the encoding
    emb = factor.embed({factor.count_key: X}, nsamples=args.cluster_draws)["mean"]
    res = factor.silhouette(emb, labels, n_clusters)
    np.save(path, res["silhouette"].cpu().numpy())
    means = ", ".join(f"{v:.3f}" for v in res["cluster_mean"].tolist())
    print(f"silhouette: {res['score']:.4f} over {res['n_scored']} cells; per cluster {means}")


def umap_cells(factor, X, path, args, start=None):
    """The 2-D map of the cells (``umap`` on the encoding that ``cluster_cells`` works on: the same seed, the same
    draws): the coordinates as a file.  ``start``: (what ``_cell_graph`` returned, the start of ``paga_cells``) for
    --umap-init paga."""
    import torch
    if args.umap_init == "paga":
        (emb, nn, g), init = start
        res = factor.graph_layout(g, init=init, n_epochs=args.umap_epochs, min_dist=args.umap_min_dist,
                                  seed=args.cluster_seed)
        res.update(graph=g, latent=emb, indices=nn["indices"], distances=nn["distances"])
    elif args.umap_init == "spectral":
        res = _umap_from_spectral(factor, X, args)
    else:
        torch.manual_seed(args.cluster_seed)              # the posterior draws of the encoding
        res = factor.umap({factor.count_key: X}, k=args.umap_neighbors, nsamples=args.cluster_draws,
                          n_epochs=args.umap_epochs, min_dist=args.umap_min_dist, seed=args.cluster_seed)
    y = res["embedding"].cpu().numpy()
    np.save(path, y)
    ok = np.isfinite(y).all(1)
    span = np.abs(y[ok]).max() if ok.any() else float("nan")
    print(f"umap: {y.shape[0]} cells, {int(res['graph']['indices'].numel())} graph entries, {res['n_epochs']} "
          f"epochs, a = {res['a']:.4f}, b = {res['b']:.4f}, extent {span:.3g}"
          + (f", {int((~ok).sum())} cells without a position" if not ok.all() else ""))
    return res


def _cell_graph(factor, X, args):
    """The encoding ``cluster_cells`` works on (the same seed, the same draws), its neighbours and their fuzzy graph:
    the first three of ``umap``'s four calls -> (latent, knn result, graph)."""
    import torch
    torch.manual_seed(args.cluster_seed)                  # the posterior draws of the encoding
    emb = factor.embed({factor.count_key: X}, nsamples=args.cluster_draws)["mean"]
    nn = factor.knn(emb, k=args.umap_neighbors)
    return emb, nn, factor.fuzzy_graph(nn["indices"], nn["distances"])


def _umap_from_spectral(factor, X, args):
    """``umap``'s four calls by hand with the spectral start between the third and the fourth -> what ``umap``
    returns (the dict ``map_cells`` needs)."""
    from spmf_amd import spectral
    emb, nn, g = _cell_graph(factor, X, args)
    eig = factor.spectral(g, n_components=2, seed=args.cluster_seed)
    start = spectral.layout_init(eig["embedding"], seed=args.cluster_seed)
    res = factor.graph_layout(g, init=start, n_epochs=args.umap_epochs, min_dist=args.umap_min_dist,
                              seed=args.cluster_seed)
    res.update(graph=g, latent=emb, indices=nn["indices"], distances=nn["distances"])
    print(f"umap: spectral start after {eig['n_iter']} iterations and {eig['n_products']} products"
          + ("" if eig["converged"] else " (not converged)"))
    return res


def spectral_cells(factor, X, path, values_path, args):
    """The spectral embedding of the cells (``spectral`` on the fuzzy graph ``umap_cells`` lays out): the
    eigenvectors and the eigenvalues as files."""
    _, _, g = _cell_graph(factor, X, args)
    res = factor.spectral(g, n_components=args.spectral, seed=args.cluster_seed)
    np.save(path, res["embedding"].cpu().numpy())
    np.save(values_path, np.asarray(res["values"], dtype=np.float64))
    print(f"spectral: {args.spectral} eigenvectors of {int(g['indices'].numel())} graph entries after "
          f"{res['n_iter']} iterations and {res['n_products']} products, largest residual "
          f"{float(res['residuals'].max()):.2e}" + ("" if res["converged"] else " (not converged)")
          + f", {res['n_unit']} eigenvalues at 1")


def community_cells(factor, X, graph, path, args):
    """Louvain clustering of the cells (``communities`` on the fuzzy graph ``umap_cells`` lays out; ``graph``: that
    graph where the layout was made, else None and it is built here): the labels as a file; -> (the labels on the
    device, as ``group_means`` and ``silhouette`` take them, and how many communities there are)."""
    if graph is None:
        _, _, graph = _cell_graph(factor, X, args)
    res = factor.communities(graph, resolution=args.resolution)
    np.save(path, res["labels"].cpu().numpy())
    sizes = ", ".join(str(n) for n in res["sizes"].tolist())
    alone = int((res["labels"] < 0).sum())
    print(f"communities: {res['n_communities']} at resolution {res['resolution']:g}, modularity "
          f"{res['modularity']:.6f}, sweeps per level {[lv['n_sweeps'] for lv in res['levels']]}, cells {sizes}"
          + (f", {alone} without a community" if alone else ""))
    return res["labels"], res["n_communities"]


def paga_cells(factor, graph, labels, n_groups, conn_path, tree_path, pos_path, args):
    """The coarse graph of the groups (``paga_init`` on the fuzzy graph ``umap_cells`` lays out): the connectivities,
    their spanning forest and the groups' positions as files; -> the start of a layout of the cells, on the device."""
    if labels is None:
        sys.exit("--paga: no cell has a community")
    res = factor.paga_init(graph, labels, n_groups=n_groups, seed=args.cluster_seed)
    conn = res["paga"]["connectivities"].cpu().numpy()
    np.save(conn_path, conn)
    np.save(tree_path, res["paga"]["connectivities_tree"].cpu().numpy())
    np.save(pos_path, res["positions"].cpu().numpy())
    G = res["paga"]["n_groups"]
    pairs = int((np.triu(conn, 1) > 0).sum())
    kept = int((np.triu(res["paga"]["connectivities_tree"].cpu().numpy(), 1) > 0).sum())
    print(f"paga: {G} groups, {pairs} connected pairs of {G * (G - 1) // 2}, {kept} in the spanning forest"
          + (f", largest connectivity {conn.max():.3f}" if pairs else ""))
    return res["init"]


def pseudotime_cells(factor, nn, root, path, labels=None, n_groups=None, group_path=None):
    """The pseudotime of the cells from cell ``root`` (``geodesic`` on ``spmf_amd.geodesic.length_graph`` of the kNN
    result ``nn``, a dict with 'indices' and 'distances'; then ``spmf_amd.geodesic.pseudotime``) as a file; with
    ``labels`` (the groups of --paga) also the mean over every group's reached cells -> the pseudotime on the device."""
    import torch
    from spmf_amd import geodesic
    g = geodesic.length_graph(nn["indices"], nn["distances"])
    res = factor.geodesic(g, torch.tensor([root]))
    t = geodesic.pseudotime(res["distances"][:, 0])
    np.save(path, t.cpu().numpy())
    reached = torch.isfinite(t)
    print(f"pseudotime: root {root}, {int(reached.sum())} of {int(t.numel())} cells reached over "
          f"{int(g['indices'].numel())} graph entries, {res['n_sweeps']} sweeps"
          + ("" if res["converged"] else " (not converged)")
          + f", largest distance {float(res['distances'][:, 0][reached].max()) if bool(reached.any()) else 0.0:.4g}")
    if labels is not None:
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        G = int(n_groups) if n_groups is not None else max(int(lab.max()) + 1, 1)
        tn = t.cpu().numpy().astype(np.float64)
        mean = np.array([tn[(lab == a) & np.isfinite(tn)].mean() if ((lab == a) & np.isfinite(tn)).any()
                         else np.nan for a in range(G)], dtype=np.float64)
        np.save(group_path, mean)
        print("pseudotime: group means " + ", ".join(f"{v:.3f}" for v in mean.tolist()))
    return t


def map_cells(factor, X_new, reference, labels, n_classes, path, label_path, args):
    """New cells on the map of ``umap_cells`` (``umap_transform`` with the same seed and draws: the map itself
    stays as written): their coordinates as a file and, with ``labels`` of the mapped-on cells, the voted labels."""
    import torch
    torch.manual_seed(args.cluster_seed)                  # the posterior draws of the encoding
    res = factor.umap_transform({factor.count_key: X_new}, reference, k=args.umap_neighbors,
                                nsamples=args.cluster_draws, labels=labels, n_classes=n_classes,
                                seed=args.cluster_seed)
    y = res["embedding"].cpu().numpy()
    np.save(path, y)
    ok = np.isfinite(y).all(1)
    line = f"umap map: {y.shape[0]} new cells on {reference['embedding'].shape[0]}, {res['n_epochs']} epochs"
    if not ok.all():
        line += f", {int((~ok).sum())} cells without a position"
    if labels is not None:
        voted = res["labels"].cpu().numpy()
        np.save(label_path, voted)
        share = res["label_share"].cpu().numpy()
        line += (f", {int((voted >= 0).sum())} labelled, mean share of the winning label "
                 f"{float(np.nanmean(share)) if (voted >= 0).any() else float('nan'):.3f}")
    print(line)


def group_table(factor, X, labels, gene_names, path, args, n_groups=None):
    """The marker-gene table: group means over the posterior draws and the log fold change of every group
    against the rest."""
    from spmf_amd import groups
    res = factor.group_means({factor.count_key: X}, labels, n_groups=n_groups, nsamples=args.group_draws)
    np.save(path, res["mean"].cpu().numpy())
    count = res["count"].cpu().numpy()
    filled = [g for g in range(len(count)) if count[g] > 0]
    for g in filled:
        rest = tuple(h for h in filled if h != g)
        if not rest:
            print(f"group {g} ({count[g]} cells): no other group to compare with")
            continue
        c = groups.contrast(res, g, rest)
        lfc, share = c["lfc"].cpu().numpy(), c["p_abs_gt"].cpu().numpy()
        sd = c["sd"].cpu().numpy() if "sd" in c else np.zeros_like(lfc)
        top = np.argsort(lfc)[::-1][:args.top]
        print(f"group {g} ({count[g]} cells): " + ", ".join(
            f"{gene_names[j]}({lfc[j]:+.2f}+-{sd[j]:.2f}, {share[j]:.2f})" for j in top))


if __name__ == "__main__":
    main()
