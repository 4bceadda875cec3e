"""What the device build's finish (MIRT_OPT_BUILD_FINISH) must report for a
tree, derived from the host builder's tree alone: shared by
test_build_finish_abi.py (pinned there, without a GPU) and test_build_finish.py."""
import numpy as np

SKIP_MASK = 0x7FFFFFFF


def node_levels(nodes):
    """Tree level of every node of a flat pre-order tree (root 0)."""
    skip = (nodes["skip"] & SKIP_MASK).astype(np.int64)
    sphere = nodes["sphere"]
    level = np.zeros(len(nodes), np.int32)
    for i in range(len(nodes)):
        if sphere[i] < 0:                       # inner: left child i + 1, right child at the left one's skip
            level[i + 1] = level[i] + 1
            level[skip[i + 1]] = level[i] + 1
    return level


def node_ranges(nodes, end):
    """Spheres of every node's subtree: from the first leaf sphere of the
    subtree up to that of the node at `skip` (`end`, one past the last sphere
    built over, where the subtree is the array's last)."""
    nn = len(nodes)
    skip = (nodes["skip"] & SKIP_MASK).astype(np.int64)
    leaves = np.flatnonzero(nodes["sphere"] >= 0)
    first = nodes["sphere"][leaves[np.searchsorted(leaves, np.arange(nn))]].astype(np.int64)
    hi = np.where(skip < nn, first[np.minimum(skip, nn - 1)], end)
    return hi - first


def finish_expect(nodes, F, end):
    """mirt_build_finish_stats' round, subtrees and nodes, and the `levels` of
    the build statistics, for the tree `nodes` (host builder) over spheres up to
    `end`, with the finish taking ranges of at most F (0: off).
    round: the least level with inner nodes whose inner nodes all hold at most F
    spheres; subtrees: the inner nodes there; nodes: the nodes deeper than that
    level plus `subtrees`; levels: round + 1, or every level of the tree."""
    level = node_levels(nodes)
    rng = node_ranges(nodes, end)
    inner = nodes["sphere"] < 0
    depth = int(level.max()) + 1 if len(nodes) else 1
    if F > 0:
        for l in range(depth):
            at = inner & (level == l)
            if not at.any():
                break
            if rng[at].max() <= F:
                return dict(round=l, subtrees=int(at.sum()), nodes=int((level > l).sum() + at.sum()), levels=l + 1)
    return dict(round=-1, subtrees=0, nodes=0, levels=depth)
