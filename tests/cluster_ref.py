"""The reference of every clustering test: the two rules of aligner_amd/csrc/aln_cluster_rules.h in plain Python.

components: a union-find with smallest-member labels.  greedy: the sequential walk in priority order.  All outputs are integers; the
tests compare them exactly.
"""
NONE = 0xFFFFFFFF
COMPONENTS, GREEDY = 0, 1


def before(len_u, u, len_v, v):
    """does u come before v in priority order?"""
    return len_u > len_v or (len_u == len_v and u < v)


def key(length, index):
    """the packed priority: the larger key comes first"""
    return (int(length) << 32) | (~int(index) & 0xFFFFFFFF)


def key_index(k):
    return ~int(k) & 0xFFFFFFFF


def is_node(v, q_first, q_count, t_first, t_count):
    return q_first <= v < q_first + q_count or t_first <= v < t_first + t_count


def node_count(q_first, q_count, t_first, t_count):
    return len(set(range(q_first, q_first + q_count)) | set(range(t_first, t_first + t_count)))


def _lengths(n, lengths):
    return [0] * n if lengths is None else [int(x) for x in lengths]


def components(n, a, b, nodes=None):
    """label per node number 0 .. n - 1 (NONE outside `nodes`, default all): the smallest node of its connected component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(a, b):
        ru, rv = find(int(u)), find(int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)       # the smaller root stays: a root is its tree's smallest member
    inside = set(range(n)) if nodes is None else set(nodes)
    return [find(v) if v in inside else NONE for v in range(n)]


def greedy(n, a, b, lengths=None, nodes=None):
    """label per node: itself for a representative, else the first representative, in priority order, it shares an edge with"""
    ln = _lengths(n, lengths)
    inside = sorted(range(n) if nodes is None else nodes)
    adj = {}
    for u, v in zip(a, b):
        u, v = int(u), int(v)
        if u != v:
            adj.setdefault(u, set()).add(v)
            adj.setdefault(v, set()).add(u)
    label = [NONE] * n
    for v in sorted(inside, key=lambda x: (-ln[x], x)):
        # (every node labelled so far comes before v: the neighbours that are their own label are the representatives before v)
        mine = [r for r in adj.get(v, ()) if label[r] == r]
        label[v] = min(mine, key=lambda r: (-ln[r], r)) if mine else v
    return label


def labels(mode, n, a, b, lengths=None, nodes=None):
    return components(n, a, b, nodes) if mode == COMPONENTS else greedy(n, a, b, lengths, nodes)


def records(label, a, b, lengths=None):
    """[(label, size, longest, edges)] in ascending label"""
    n = len(label)
    ln = _lengths(n, lengths)
    size, longest, edges = {}, {}, {}
    for v, l in enumerate(label):
        if l == NONE:
            continue
        size[l] = size.get(l, 0) + 1
        if l not in longest or before(ln[v], v, ln[longest[l]], longest[l]):
            longest[l] = v
    for u, v in zip(a, b):
        u, v = int(u), int(v)
        if u != v and label[u] == label[v]:
            edges[label[u]] = edges.get(label[u], 0) + 1
    return [(l, size[l], longest[l], edges.get(l, 0)) for l in sorted(size)]


def summary(label, recs, a, b):
    """the summary's fields but `rounds` (how many rounds the device took is its own business)"""
    self_edges = sum(1 for u, v in zip(a, b) if int(u) == int(v))
    return dict(nodes=sum(1 for l in label if l != NONE), clusters=len(recs), edges=len(a) - self_edges, self_edges=self_edges,
                singletons=sum(1 for r in recs if r[1] == 1))


def members(label, recs):
    """node numbers per cluster, clusters in record order, ascending within a cluster"""
    by = {r[0]: [] for r in recs}
    for v, l in enumerate(label):
        if l != NONE:
            by[l].append(v)
    return [by[r[0]] for r in recs]


def cluster(mode, n, a, b, lengths=None, nodes=None):
    """(label, records, summary, members) of one call"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    lab = labels(mode, n, a, b, lengths, nodes)
    recs = records(lab, a, b, lengths)
    return lab, recs, summary(lab, recs, a, b), members(lab, recs)
