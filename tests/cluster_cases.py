"""Not a test: what the clustering tests share.

cluster_reference is the plain-Python statement of vi_indexer_cluster_radius's definition (include/vi_amd.h): rows of the
radius graph -> (labels, degree, n_clusters), by a sequential union-find over the edges read in both directions, the
border records taking their lowest adjacent core ordinal.  planted builds the data set the GPU tests cluster."""
import numpy as np

NOISE = -1      # VI_LABEL_NOISE


def cluster_reference(rows, n, min_pts, participant=None):
    """rows[j]: the ordinals of row j's hits (any order, duplicates and j itself tolerated and ignored) — read only for
    participants; participant: bool[n] or None (everyone).  Returns (labels i64[n], degree u32[n], n_clusters, counts),
    counts = {"n_core", "n_border", "n_noise", "hits"}."""
    part = np.ones(n, dtype=bool) if participant is None else np.asarray(participant, dtype=bool)
    R = [set() for _ in range(n)]
    for j in range(n):
        if part[j]:
            R[j] = {int(b) for b in rows[j]} - {j}
            assert all(part[b] for b in R[j]), "a hit that is no participant: the filter deletes those"
    degree = np.array([len(r) for r in R], dtype=np.uint32)
    core = part & (degree.astype(np.int64) + 1 >= int(min_pts))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    border = {}
    for a in range(n):
        for b in R[a]:          # a ~ b: whichever row holds the pair
            if core[a] and core[b]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)     # the root is the component's minimum
            elif core[a]:
                border[b] = min(border.get(b, a), a)
            elif core[b]:
                border[a] = min(border.get(a, b), b)
    labels = np.full(n, NOISE, dtype=np.int64)
    for j in range(n):
        if core[j]:
            labels[j] = find(j)
    for j, c in border.items():
        assert part[j] and not core[j]
        labels[j] = find(c)
    members = {}
    for j in np.nonzero(core)[0]:
        members.setdefault(int(labels[j]), []).append(int(j))
    assert all(min(m) == r for r, m in members.items())           # labels[j] == j exactly for the representatives
    counts = {"n_core": int(core.sum()), "n_border": len(border), "n_noise": int(part.sum()) - int(core.sum()) - len(border),
              "hits": int(degree.sum())}
    return labels, degree, len(members), counts


def cluster_reference_csr(lims, cols, n, min_pts, participant=None):
    """The same definition for rows too large for a Python loop (every probed record at radius +inf: millions of
    entries), in numpy: rows in CSR form (row j owns cols[lims[j]:lims[j + 1]], each hit once), the components by
    min-label propagation with pointer jumping instead of a union-find.  test_cluster_rules_cpu.py holds it to
    cluster_reference on random and hand-made graphs; the results are identical by construction of the definition."""
    part = np.ones(n, dtype=bool) if participant is None else np.asarray(participant, dtype=bool)
    lims, cols = np.asarray(lims, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(lims))
    keep = part[a] & (cols != a)
    a, b = a[keep], cols[keep]
    assert part[b].all(), "a hit that is no participant: the filter deletes those"
    degree = np.bincount(a, minlength=n).astype(np.uint32)
    core = part & (degree.astype(np.int64) + 1 >= int(min_pts))
    both = core[a] & core[b]
    ea, eb = a[both], b[both]
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = lab.copy()
        np.minimum.at(m, ea, lab[eb])
        np.minimum.at(m, eb, lab[ea])
        m = m[m]                    # (m[x] <= x is a member of x's component: so is its label)
        if np.array_equal(m, lab):
            break
        lab = m
    border = np.full(n, n, dtype=np.int64)
    one = core[a] & ~core[b]
    np.minimum.at(border, b[one], a[one])
    one = ~core[a] & core[b]
    np.minimum.at(border, a[one], b[one])
    is_border = border < n
    labels = np.full(n, NOISE, dtype=np.int64)
    labels[core] = lab[core]
    labels[is_border] = lab[border[is_border]]
    counts = {"n_core": int(core.sum()), "n_border": int(is_border.sum()),
              "n_noise": int(part.sum()) - int(core.sum()) - int(is_border.sum()), "hits": int(degree.sum())}
    return labels, degree, int(np.unique(labels[core]).size), counts


# ---- the planted data set (eps^2 = 1) ----
DIM, NLIST, NBACKGROUND, NCHAIN, NWALK, NLEAVES, NCOPIES = 32, 24, 3000, 200, 200, 30, 70
EPS2 = 1.0


def planted(seed=1):
    """(X f32[n, 32], parts): 3000 standard-normal background rows and, far from them and from each other, a straight
    chain of 200 points 0.9 apart, a 200-step random walk of step 0.9, two stars (hub + 30 leaves at hub + 0.8 e_i, the
    hubs 1.5 e_31 apart), one bridge point at hub1 + 0.75 e_31 and one vector stored 70 times; all rows shuffled.
    parts: name -> the rows (of X) of that shape."""
    rng = np.random.default_rng(seed)
    e = np.eye(DIM)
    chain = 25.0 * e[1] + 0.9 * np.arange(NCHAIN)[:, None] * e[0][None, :]
    steps = rng.standard_normal((NWALK, DIM))
    steps *= 0.9 / np.linalg.norm(steps, axis=1, keepdims=True)
    walk = -25.0 * e[2] + np.cumsum(steps, axis=0)
    hub1 = 25.0 * e[3] + 25.0 * e[4]
    hub2 = hub1 + 1.5 * e[31]
    star1 = np.concatenate([hub1[None], hub1[None] + 0.8 * e[:NLEAVES]])
    star2 = np.concatenate([hub2[None], hub2[None] + 0.8 * e[:NLEAVES]])
    bridge = (hub1 + 0.75 * e[31])[None]
    copies = np.repeat(rng.standard_normal((1, DIM)), NCOPIES, axis=0)
    blocks = [("background", rng.standard_normal((NBACKGROUND, DIM))), ("chain", chain), ("walk", walk), ("star1", star1),
              ("star2", star2), ("bridge", bridge), ("copies", copies)]
    X = np.concatenate([b for _, b in blocks]).astype(np.float32)
    perm = rng.permutation(X.shape[0])
    where = np.empty_like(perm)
    where[perm] = np.arange(perm.size)          # row i of the unshuffled set is row where[i] of X[perm]
    parts, at = {}, 0
    for name, b in blocks:
        parts[name] = np.sort(where[at:at + b.shape[0]])
        at += b.shape[0]
    parts["hub1"], parts["hub2"] = where[NBACKGROUND + NCHAIN + NWALK], where[NBACKGROUND + NCHAIN + NWALK + 1 + NLEAVES]
    return np.ascontiguousarray(X[perm]), parts
