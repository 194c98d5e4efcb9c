"""Hand-built trees (inputs only, pure NumPy; no product logic here): edits of a tests/util.make_problem dict that keep it a
valid problem of the class st_create documents -- `indexing` an ascending partition of the rows, `parents` ascending
chains with parents(u) = parents(last parent) + [last parent] (one parent per block for limited_tree), every parent an
observed block of a shallower reference level, `children` all observed descendants (limited_tree: the observed direct
children) -- but of shapes topology.prepare never builds: blocks of one level behind chains of different lengths, sibling
blocks of any widths, empty blocks, reference blocks with none or many direct children.

The edits (rehang, reparent, move_rows, rehang_limited) assert their preconditions and end in check_problem: none of them
silently builds a tree that st_create ought to refuse.  SHAPES are named problems built from them; each asserts, from the
problem alone, the property it is named for.
"""
import numpy as np

from tests.util import make_problem


# ---- reading a problem
def n_blocks(pb):
    return len(pb["indexing"])


def level_of(pb, u):
    """Index of u's level among the sorted level labels (what res_is_ref is indexed by)."""
    return int(np.searchsorted(np.unique(pb["block_groups"]), pb["block_groups"][u]))


def is_reference_level(pb, u):
    return int(pb["res_is_ref"][level_of(pb, u)]) == 1


def n_observed(pb, u):
    return int(np.isfinite(pb["y"][pb["indexing"][u]]).sum())


def blocks_of_level(pb, g):
    return [u for u in range(n_blocks(pb)) if level_of(pb, u) == g]


def last_parent(pb, u):
    return int(pb["parents"][u][-1]) if len(pb["parents"][u]) else -1


def direct_children(pb, a, observed_only=False):
    return [u for u in range(n_blocks(pb)) if last_parent(pb, u) == a and (n_observed(pb, u) > 0 or not observed_only)]


def subtree(pb, u):
    """The blocks below u (u itself not included)."""
    if not pb.get("limited_tree", False):
        return [v for v in range(n_blocks(pb)) if u in pb["parents"][v]]
    out, front = [], [u]
    while front:
        front = [v for v in range(n_blocks(pb)) if last_parent(pb, v) in front]
        out += front
    return sorted(out)


def rebuild_children(pb):
    """children(a) from parents: every observed block that lists a (limited_tree: whose single parent is a), ascending."""
    ch = [[] for _ in range(n_blocks(pb))]
    for u in range(n_blocks(pb)):
        if n_observed(pb, u) > 0:
            for a in pb["parents"][u]:
                ch[int(a)].append(u)
    pb["children"] = [np.asarray(sorted(c), dtype=np.int64) for c in ch]


def check_problem(pb):
    """The documented class, asserted: what every edit must leave behind."""
    nb, limited = n_blocks(pb), pb.get("limited_tree", False)
    rows = np.concatenate(pb["indexing"])
    assert np.array_equal(np.sort(rows), np.arange(pb["n"])), "indexing is not a partition of the rows"
    want = [[] for _ in range(nb)]
    for u in range(nb):
        ix, pa = np.asarray(pb["indexing"][u]), np.asarray(pb["parents"][u])
        assert np.all(np.diff(ix) > 0) and np.all(np.diff(pa) > 0), u
        assert np.all(pb["blocking"][ix] == u + 1), u
        for a in pa:
            assert level_of(pb, a) < level_of(pb, u) and is_reference_level(pb, a), (u, a)
            assert n_observed(pb, a) > 0, ("ancestor without observed rows", u, a)
        if limited:
            assert pa.size <= 1, u
        elif pa.size:
            assert np.array_equal(pa[:-1], pb["parents"][pa[-1]]), ("chain rule", u)
        if n_observed(pb, u) > 0:
            for a in pa:
                want[int(a)].append(u)
    for u in range(nb):
        assert list(pb["children"][u]) == sorted(want[u]), ("children", u)
        assert not want[u] or (is_reference_level(pb, u) and n_observed(pb, u) > 0), ("children of a non-reference block", u)


# ---- the edits
def rehang(pb, u, drop=1):
    """u and its whole subtree lose the `drop` ancestors just above u: u then hangs from a shallower reference level."""
    assert not pb.get("limited_tree", False), "rehang_limited is the limited-tree variant"
    pa = [int(a) for a in pb["parents"][u]]
    assert 1 <= drop < len(pa), (u, drop, pa)      # u keeps a parent
    gone = set(pa[-drop:])
    for v in [u] + subtree(pb, u):
        pb["parents"][v] = np.asarray([a for a in pb["parents"][v] if int(a) not in gone], dtype=np.int64)
    rebuild_children(pb)
    check_problem(pb)


def reparent(pb, u, new_parent):
    """u and its subtree move under another observed reference block of a shallower level."""
    assert not pb.get("limited_tree", False)
    assert level_of(pb, new_parent) < level_of(pb, u) and is_reference_level(pb, new_parent), (u, new_parent)
    assert n_observed(pb, new_parent) > 0 and new_parent != u and new_parent not in subtree(pb, u), (u, new_parent)
    old = set(int(a) for a in pb["parents"][u])
    chain = [int(a) for a in pb["parents"][new_parent]] + [int(new_parent)]
    for v in [u] + subtree(pb, u):
        pb["parents"][v] = np.asarray(chain + [int(a) for a in pb["parents"][v] if int(a) not in old], dtype=np.int64)
    rebuild_children(pb)
    check_problem(pb)


def rehang_limited(pb, u):
    """limited_tree: u's single parent becomes its grandparent (u's own subtree still hangs from u)."""
    assert pb.get("limited_tree", False)
    assert len(pb["parents"][u]) == 1
    gp = pb["parents"][last_parent(pb, u)]
    assert len(gp) == 1, (u, "its parent is a root")
    pb["parents"][u] = np.asarray(gp, dtype=np.int64).copy()
    rebuild_children(pb)
    check_problem(pb)


def move_rows(pb, src, dst, k):
    """The last k rows of block src go to block dst of the same level (k = "all" empties src).  A block that loses its last
    observed row must have nothing below it."""
    assert src != dst and level_of(pb, src) == level_of(pb, dst), (src, dst)
    ix = np.asarray(pb["indexing"][src])
    k = ix.size if k == "all" else int(k)
    assert 1 <= k <= ix.size, (src, k, ix.size)
    moved = ix[ix.size - k:]
    pb["indexing"][src] = ix[:ix.size - k].copy()
    pb["indexing"][dst] = np.sort(np.concatenate([pb["indexing"][dst], moved])).astype(np.int64)
    pb["blocking"] = np.asarray(pb["blocking"]).copy()
    pb["blocking"][moved] = dst + 1
    assert n_observed(pb, src) > 0 or not subtree(pb, src), ("an ancestor would be left without observed rows", src)
    rebuild_children(pb)
    check_problem(pb)


def set_widths(pb, blocks, widths):
    """Blocks of one level get the given numbers of rows (the same total), by move_rows between them."""
    have = [len(pb["indexing"][u]) for u in blocks]
    assert sum(have) == sum(widths) and len(blocks) == len(widths), (have, widths)
    for i, u in enumerate(blocks):
        for j, v in enumerate(blocks):
            k = min(len(pb["indexing"][u]) - widths[i], widths[j] - len(pb["indexing"][v]))
            if i != j and k > 0:
                move_rows(pb, u, v, k)
    assert [len(pb["indexing"][u]) for u in blocks] == list(widths)


def widen(pb, u, width, donors):
    """Block u grows to `width` rows, one row at a time from the `donors` (same level), each of which keeps a row."""
    for v in donors:
        while len(pb["indexing"][u]) < width and v != u and len(pb["indexing"][v]) > 1:
            move_rows(pb, v, u, 1)
    assert len(pb["indexing"][u]) == width, (u, width)


# ---- reading the shapes
def leaf_level(pb):
    """The deepest level with observed blocks."""
    return max(level_of(pb, u) for u in range(n_blocks(pb)) if n_observed(pb, u) > 0)


def chain_lengths(pb, g):
    return sorted(set(len(pb["parents"][u]) for u in blocks_of_level(pb, g) if len(pb["indexing"][u])))


def child_groups(pb, a):
    """The widths of the column groups the observed direct children of a (all non-reference blocks) fall into: in id order,
    consecutive siblings of at most 32 columns and 32 blocks per group."""
    groups, nblk = [], 0
    for u in direct_children(pb, a, observed_only=True):
        m = len(pb["indexing"][u])
        if groups and groups[-1] + m <= 32 and nblk < 32:
            groups[-1] += m
            nblk += 1
        else:
            groups.append(m)
            nblk = 1
    return groups


def every_third(blocks):
    return blocks[1::3]


# ---- the shapes.  Base problems: seed 11, as tests/test_gpu_routes.build_problem makes them
def mixed_chain_leaf(side=25, q=1, **kw):
    """Every third leaf block hangs from its grandparent: the leaf level holds chains of two lengths, and reference blocks
    have direct children on two levels."""
    pb = make_problem(side=side, q=q, seed=11, **kw)
    g = leaf_level(pb)
    assert not is_reference_level(pb, blocks_of_level(pb, g)[0])
    for u in every_third(blocks_of_level(pb, g)):
        rehang(pb, u)
    lens = chain_lengths(pb, g)
    assert len(lens) == 2 and lens[1] == lens[0] + 1, lens
    two = [a for a in range(n_blocks(pb)) if len(set(level_of(pb, c) for c in direct_children(pb, a, True))) == 2]
    assert two, "no reference block with direct children on two levels"
    return pb


def mixed_chain_ref():
    """One level-3 reference block, with its leaves, hangs from the root: the reference level has mixed chain lengths, and
    the leaves under that block have a chain without the level-2 block."""
    pb = make_problem(side=25, q=1, seed=11)
    u = blocks_of_level(pb, 2)[5]
    skipped = last_parent(pb, u)
    leaves = direct_children(pb, u)
    rehang(pb, u)
    assert chain_lengths(pb, 2) == [1, 2] and last_parent(pb, u) == blocks_of_level(pb, 0)[0]
    assert leaves and all(list(pb["parents"][v]) == [last_parent(pb, u), u] and skipped not in pb["parents"][v] for v in leaves)
    assert chain_lengths(pb, 3) == [2, 3]
    return pb


def uneven_widths():
    """Sibling reference blocks of 1, 31, 32 and of 16, 17 rows (the column-group limits: tiles of 16, the 16 + 11 blocked
    elimination, the wave elimination up to 27 rows, 32 columns); under one parent, leaf blocks of 1 row that fill a column
    group to exactly 32 columns; under another, leaves of 33 columns that split into two groups."""
    pb = make_problem(side=25, q=1, seed=11)
    l2 = blocks_of_level(pb, 1)
    fam_a, fam_b = direct_children(pb, l2[0]), direct_children(pb, l2[1])
    tot_a, tot_b = (sum(len(pb["indexing"][u]) for u in fam) for fam in (fam_a, fam_b))
    set_widths(pb, fam_a, [1, 31, 32, tot_a - 64])
    rest = tot_b - 33
    set_widths(pb, fam_b, [16, 17, rest // 2, rest - rest // 2])
    widths = sorted(len(pb["indexing"][u]) for u in fam_a + fam_b)
    assert {1, 16, 17, 31, 32} <= set(widths) and widths[-1] == 32, widths
    assert all(last_parent(pb, u) == l2[0] for u in fam_a) and all(last_parent(pb, u) == l2[1] for u in fam_b)
    # leaves: the children of the 32-row block fill one group of exactly 32 columns, with 1-row blocks among them; those of
    # the 1-row block make 33 columns: two groups
    leaves = blocks_of_level(pb, 3)
    for parent, total in ((fam_a[2], 32), (fam_a[0], 33)):
        sibs = direct_children(pb, parent)
        donors = [v for v in leaves if last_parent(pb, v) not in (fam_a[2], fam_a[0])]
        for v in sibs[1:]:
            if len(pb["indexing"][v]) > 1:
                move_rows(pb, v, sibs[0], len(pb["indexing"][v]) - 1)
        widen(pb, sibs[0], total - (len(sibs) - 1), donors)
    assert child_groups(pb, fam_a[2]) == [32] and len(child_groups(pb, fam_a[0])) == 2 and sum(child_groups(pb, fam_a[0])) == 33
    assert min(len(pb["indexing"][v]) for v in direct_children(pb, fam_a[2])) == 1
    assert max(len(pb["indexing"][u]) for u in range(n_blocks(pb))) <= 32
    return pb


def one_row_and_wide():
    """Reference blocks of 1 and 45 rows in one level: too wide for the column groups, the level (and the leaf level behind
    it) goes to k_factor_lchain, with slabs of unequal chain length and row stride."""
    pb = make_problem(side=25, q=1, seed=11)
    fam = direct_children(pb, blocks_of_level(pb, 1)[0])
    tot = sum(len(pb["indexing"][u]) for u in fam)
    rest = tot - 46
    set_widths(pb, fam, [1, 45, rest // 2, rest - rest // 2])
    widths = [len(pb["indexing"][u]) for u in blocks_of_level(pb, 2)]
    assert min(widths) == 1 and max(widths) == 45
    return pb


def empty_and_childless(missing=0.12):
    """An emptied leaf block, a reference block with no children at all, and a reference block whose only children are NA
    (prediction) blocks.  missing=0: every row observed (what st_simulate asks for), so the third block is bare as well."""
    pb = make_problem(side=25, q=1, seed=11, missing=missing)
    l3 = blocks_of_level(pb, 2)
    bare, na_only, host = l3[3], l3[9], l3[4]
    for v in direct_children(pb, bare):
        reparent(pb, v, host)
    for v in direct_children(pb, na_only, observed_only=True):
        reparent(pb, v, host)
    leaves = direct_children(pb, l3[0], observed_only=True)
    move_rows(pb, leaves[0], leaves[1], "all")
    assert len(pb["indexing"][leaves[0]]) == 0
    assert direct_children(pb, bare) == [] and len(pb["children"][bare]) == 0
    kids = direct_children(pb, na_only)
    assert (kids or not missing) and all(n_observed(pb, v) == 0 and len(pb["indexing"][v]) for v in kids) and len(pb["children"][na_only]) == 0
    pb["emptied"] = leaves[0]
    return pb


def many_children(n_wide):
    """The leaves of three sibling parents re-parented under a fourth; `n_wide` of them widened to 17 rows (two such
    blocks do not share a column group) and the rest narrowed to one row, so that the fourth parent has exactly `n_wide`
    direct child groups: 4 is the most k_gram_direct takes (GRAM_DIRECT_MAXCH), 5 must turn that route off."""
    pb = make_problem(side=25, q=1, seed=11)
    fam = direct_children(pb, blocks_of_level(pb, 1)[2])
    host = fam[0]
    for a in fam[1:]:
        for v in direct_children(pb, a):
            reparent(pb, v, host)
    kids = direct_children(pb, host)
    assert len(kids) >= 12
    others = [v for v in blocks_of_level(pb, 3) if v not in kids]
    for v in kids[n_wide:]:
        if len(pb["indexing"][v]) > 1:
            move_rows(pb, v, kids[0], len(pb["indexing"][v]) - 1)
    for v in kids[:n_wide]:
        if len(pb["indexing"][v]) > 17:
            move_rows(pb, v, others[0], len(pb["indexing"][v]) - 17)
        widen(pb, v, 17, others)
    groups = child_groups(pb, host)
    assert len(groups) == n_wide and groups[:n_wide - 1] == [17] * (n_wide - 1), groups
    assert all(len(child_groups(pb, a)) <= 1 for a in blocks_of_level(pb, 2) if a != host)
    assert all(direct_children(pb, a) == [] for a in fam[1:])
    pb["host"] = host
    return pb


def na_blocks_rehung():
    """Prediction blocks hanging from levels 1 and 2 as well as from the last reference level; one of them shares its
    (level-2) parent with an observed leaf."""
    pb = make_problem(side=25, q=1, seed=11, missing=0.12)
    na = [u for u in range(n_blocks(pb)) if n_observed(pb, u) == 0]
    assert na and all(len(pb["indexing"][u]) and len(pb["parents"][u]) == 3 for u in na)
    for i, u in enumerate(na):
        if i % 3 < 2:
            rehang(pb, u, drop=2 - i % 3)
    assert sorted(set(level_of(pb, last_parent(pb, u)) for u in na)) == [0, 1, 2]
    shared = last_parent(pb, na[1])       # a level-2 block
    assert level_of(pb, shared) == 1
    leaf = [v for v in blocks_of_level(pb, 3) if shared in pb["parents"][v]][0]
    rehang(pb, leaf)
    both = direct_children(pb, shared)
    assert leaf in both and na[1] in both and n_observed(pb, leaf) > 0
    return pb


def wide_mixed():
    """Side 12, three outcomes (blocks of up to 75 rows: the wide-block path): every third leaf hangs from the root, and 5
    rows move between two level-2 blocks."""
    pb = mixed_chain_leaf(side=12, q=3)
    l2 = blocks_of_level(pb, 1)
    before = [len(pb["indexing"][u]) for u in l2[:2]]
    move_rows(pb, l2[0], l2[1], 5)
    assert [len(pb["indexing"][u]) for u in l2[:2]] == [before[0] - 5, before[1] + 5]
    assert max(len(pb["indexing"][u]) for u in range(n_blocks(pb))) > 64
    return pb


def two_outcomes_mixed():
    """Side 16, two outcomes (50-row reference blocks): every third leaf hangs from the root; level-2 blocks of 31, 69, 33
    and 67 rows; a leaf block of one row and one of exactly 32."""
    pb = mixed_chain_leaf(side=16, q=2)
    l2 = blocks_of_level(pb, 1)
    assert sum(len(pb["indexing"][u]) for u in l2) == 200
    set_widths(pb, l2, [31, 69, 33, 67])
    leaves = blocks_of_level(pb, 2)
    a, b, c = leaves[0], leaves[3], leaves[6]
    move_rows(pb, a, c, len(pb["indexing"][a]) - 1)
    have = len(pb["indexing"][b])
    if have > 32:
        move_rows(pb, b, c, have - 32)
    widen(pb, b, 32, [v for v in leaves if v not in (a, b)])
    assert len(pb["indexing"][a]) == 1 and len(pb["indexing"][b]) == 32
    return pb


def limited_skip():
    """limited_tree: the single parent of every third leaf is its grandparent."""
    pb = make_problem(side=25, q=1, seed=11, limited_tree=True)
    g = leaf_level(pb)
    hung = every_third(blocks_of_level(pb, g))
    for u in hung:
        rehang_limited(pb, u)
    assert sorted(set(level_of(pb, last_parent(pb, u)) for u in blocks_of_level(pb, g))) == [g - 2, g - 1]
    return pb


SHAPES = {
    "mixed_chain_leaf": mixed_chain_leaf,
    "mixed_chain_ref": mixed_chain_ref,
    "uneven_widths": uneven_widths,
    "one_row_and_wide": one_row_and_wide,
    "empty_and_childless": empty_and_childless,
    "empty_all_observed": lambda: empty_and_childless(missing=0.0),
    "many_children_5": lambda: many_children(5),
    "many_children_4": lambda: many_children(4),
    "na_blocks_rehung": na_blocks_rehung,
    "wide_mixed": wide_mixed,
    "two_outcomes_mixed": two_outcomes_mixed,
    "limited_skip": limited_skip,
}
_BUILT = {}


def shape(name):
    """A fresh copy of the named problem (built once per process: the edits are many small steps)."""
    import copy
    if name not in _BUILT:
        _BUILT[name] = SHAPES[name]()
    return copy.deepcopy(_BUILT[name])
