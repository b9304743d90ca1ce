"""Reference statement of the components / cluster contract (strsim_components_*, strsim_cluster_*): a plain union-find.
components(indptr, index, rows): the edges (i, index[e]), e in [indptr[i], indptr[i + 1]), read as undirected -> (root, cluster,
count) as lists: root[v] the smallest row of v's component, cluster[v] the number of roots below it, count the number of
components.  cluster(measure, strings, min_score): the components of the upper self-join of join_ref / match_join_ref, with the
number of its pairs."""

CLUSTER_MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice", "ratio", "token_sort_ratio")
# the name Context.cluster takes
MEASURE = {m: m for m in CLUSTER_MEASURES[:5]}
MEASURE.update({"ratio": "indel", "token_sort_ratio": "token_sort_ratio"})


def components(indptr, index, rows=None):
    n = len(indptr) - 1 if rows is None else int(rows)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u in range(n):
        for e in range(int(indptr[u]), int(indptr[u + 1])):
            a, b = find(u), find(int(index[e]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = [find(v) for v in range(n)]
    rank, count = {}, 0
    for v in range(n):
        if root[v] == v:
            rank[v] = count
            count += 1
    return root, [rank[r] for r in root], count


def hits(measure, strings, min_score):
    """the upper self-join as (indptr, index, score) by the join models"""
    strings = list(strings)
    if measure in ("ratio", "token_sort_ratio"):
        import join_ref
        return join_ref.join(measure, strings, strings, min_score, True)
    import match_join_ref
    return match_join_ref.join(measure, strings, strings, min_score, True)


def cluster(measure, strings, min_score, found=None):
    """-> (root, cluster, count, nnz); found: the hits, when the caller has them already"""
    indptr, index, _ = found if found is not None else hits(measure, strings, min_score)
    return (*components(indptr, index, len(indptr) - 1), len(index))


def worth_it(measure, strings, min_score, found=None):
    """Whether a frame tests anything: at least three clusters of three or more members, and at least one cluster that holds a pair
    which is not itself a hit (the components chain)."""
    strings = list(strings)
    indptr, index, _ = found if found is not None else hits(measure, strings, min_score)
    root, _, _ = components(indptr, index, len(strings))
    members = {}
    for v, r in enumerate(root):
        members.setdefault(r, []).append(v)
    big = [m for m in members.values() if len(m) >= 3]
    edges = {(u, int(index[e])) for u in range(len(strings)) for e in range(int(indptr[u]), int(indptr[u + 1]))}
    chained = any((a, b) not in edges for m in big for x, a in enumerate(m) for b in m[x + 1:])
    return len(big) >= 3 and chained
