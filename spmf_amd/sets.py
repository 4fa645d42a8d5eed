"""What goes into ``set_scores``: the packed form of a list of column sets and a reader of the GMT gene-set
format.  Plain numpy / torch on the host layer; nothing here is on the hot path.
"""
import numpy as np
import torch


def pack(sets, weights, D, name="set_scores"):
    """The sets of ``set_scores`` (``name``) in the form the library takes, checked on the way: ``sets`` is a
    sequence of 1-D integer arrays (numpy / torch / lists) of columns inside [0, D), duplicates kept; ``weights``
    None or a sequence of as many float arrays, each as long as its set, all finite.

    -> (set_ptr: int64 numpy [G + 1] on the host, cols: int32 tensor [set_ptr[G]], weights: float32 tensor
    [set_ptr[G]] or None), the lists of the sets one behind the other."""
    from .streaming import _vector
    if isinstance(sets, (np.ndarray, torch.Tensor)) and getattr(sets, "ndim", 1) == 2:
        raise ValueError(f"{name}: sets must be a sequence of 1-D arrays, one per set (a 2-D array is ambiguous)")
    sets = list(sets)
    D = int(D)
    cols = []
    for g, s in enumerate(sets):
        t = _vector(name, f"set {g}", s).cpu().to(torch.int64)
        if t.numel():
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= D:
                raise ValueError(f"{name}: the columns of set {g} must lie in [0, {D}), got {lo} .. {hi}")
        cols.append(t)
    sizes = np.array([int(t.numel()) for t in cols], dtype=np.int64)
    set_ptr = np.zeros(len(cols) + 1, dtype=np.int64)
    np.cumsum(sizes, out=set_ptr[1:])
    flat = torch.cat(cols).to(torch.int32) if cols else torch.zeros(0, dtype=torch.int32)
    if weights is None:
        return set_ptr, flat, None
    weights = list(weights)
    if len(weights) != len(cols):
        raise ValueError(f"{name}: weights must hold one array per set, got {len(weights)} for {len(cols)} sets")
    ws = []
    for g, w in enumerate(weights):
        t = _vector(name, f"weights of set {g}", w, integer=False).cpu().to(torch.float64)
        if int(t.numel()) != int(sizes[g]):
            raise ValueError(f"{name}: the weights of set {g} must be as long as the set, got {int(t.numel())} "
                             f"for {int(sizes[g])} columns")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name}: the weights of set {g} must be finite")
        ws.append(t.to(torch.float32))
    return set_ptr, flat, torch.cat(ws) if ws else torch.zeros(0, dtype=torch.float32)


def read_gmt(path, names):
    """The sets of a GMT file (one set per line, tab-separated: set name, description, member names) as column
    indices: a member is looked up in ``names`` (the column names in column order; the first of equal names
    wins), an unknown member is dropped, a member listed twice stays twice, a set may come out empty.

    -> (set_names: list of str, sets: list of int64 numpy arrays, dropped: the number of members dropped)."""
    index = {}
    for j, n in enumerate(names):
        index.setdefault(str(n), j)
    set_names, sets, dropped = [], [], 0
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            fields = line.split("\t")
            members = [m.strip() for m in fields[2:] if m.strip()]
            found = [index[m] for m in members if m in index]
            dropped += len(members) - len(found)
            set_names.append(fields[0].strip())
            sets.append(np.array(found, dtype=np.int64))
    return set_names, sets, dropped
