"""``Rotation3D`` and small helpers (mirror of reference ``src/flygym/utils/math.py:114-175``)."""

from dataclasses import dataclass
from numbers import Number
from typing import Sequence

import numpy as np

__all__ = ["Rotation3D", "Tree", "orderedset"]

_DIMS = {"quat": 4, "axisangle": 4, "xyaxes": 6, "zaxis": 3, "euler": 3}


def orderedset(items):
    """The items without repeats, first occurrences in order."""
    return list(dict.fromkeys(items))


class Tree:
    """An undirected tree over hashable nodes (reference ``utils/math.py``: ``Tree(nodes, edges)``, ``dfs_edges(root)``).

    Construction checks that the graph really is a tree — no repeated nodes, no self loops, no parallel edges, every
    edge between known nodes, connected, acyclic — and raises ``ValueError`` otherwise.  ``dfs_edges(root)`` yields
    ``(parent, child)`` pairs in depth-first order, children in the order their edges were given."""

    def __init__(self, nodes, edges):
        self.nodes = list(nodes)
        self.edges = [tuple(e) for e in edges]
        if len(set(self.nodes)) != len(self.nodes):
            raise ValueError("Tree nodes must be unique.")
        known = set(self.nodes)
        self._adj = {n: [] for n in self.nodes}
        seen_pairs = set()
        for a, b in self.edges:
            if a not in known or b not in known:
                raise ValueError(f"Edge ({a}, {b}) refers to a node that is not in the tree.")
            if a == b or frozenset((a, b)) in seen_pairs:
                raise ValueError("Self loops and parallel edges are not allowed in a tree.")
            seen_pairs.add(frozenset((a, b)))
            self._adj[a].append(b)
            self._adj[b].append(a)
        if self.nodes:
            if len(self.edges) != len(self.nodes) - 1:
                raise ValueError("A tree over n nodes has exactly n - 1 edges (cycle or disconnected graph).")
            reached, todo = set(), [self.nodes[0]]
            while todo:
                n = todo.pop()
                if n not in reached:
                    reached.add(n)
                    todo.extend(self._adj[n])
            if len(reached) != len(self.nodes):
                raise ValueError("The graph is not connected.")

    def dfs_edges(self, root):
        if root not in self._adj:
            raise ValueError(f"Root '{root}' not in tree")
        seen = {root}
        stack = [(root, iter(self._adj[root]))]
        while stack:
            node, it = stack[-1]
            for nb in it:
                if nb not in seen:
                    seen.add(nb)
                    yield node, nb
                    stack.append((nb, iter(self._adj[nb])))
                    break
            else:
                stack.pop()


@dataclass(frozen=True)
class Rotation3D:
    format: str
    values: Sequence[Number]

    def __post_init__(self):
        ok = (
            self.format in _DIMS
            and isinstance(self.values, Sequence)
            and all(isinstance(v, Number) for v in self.values)
        )
        if not ok:
            raise ValueError(
                f"Invalid rotation spec: format={self.format}, values={self.values}. "
                f"Format must be one of {list(_DIMS)} and values must be a sequence of numbers."
            )
        if len(self.values) != _DIMS[self.format]:
            raise ValueError(
                f"Invalid rotation spec: format={self.format}, values={self.values}. "
                f"Format {self.format} should be {_DIMS[self.format]}-dimensional, got {len(self.values)}."
            )

    def as_kwargs(self):
        return {self.format: self.values}

    def as_quat(self) -> np.ndarray:
        """(w, x, y, z); only the formats the engine can spawn from."""
        if self.format == "quat":
            q = np.asarray(self.values, dtype=np.float64)
            return q / np.linalg.norm(q)
        if self.format == "axisangle":
            ax = np.asarray(self.values[:3], dtype=np.float64)
            ax = ax / np.linalg.norm(ax)
            h = 0.5 * float(self.values[3])
            return np.array([np.cos(h), *(ax * np.sin(h))])
        raise ValueError(f"cannot convert rotation format '{self.format}' to a quaternion")

    def as_matrix(self) -> np.ndarray:
        """3 x 3 rotation matrix (float64, orthonormal, right-handed) of every format MuJoCo's ``orientation`` attributes take:
        ``quat`` (w, x, y, z), ``axisangle`` (axis, angle in radians), ``xyaxes`` (the frame's x axis, then a y axis that is
        made orthogonal to it; z = x cross y), ``zaxis`` (the minimal rotation that takes (0, 0, 1) to the given direction),
        ``euler`` (the model's compiler settings, reference ``mujoco_globals.yaml:3-4``: radians, ``eulerseq: XYZ`` — rotations
        about the fixed parent axes x, then y, then z).  For a camera the columns are its right, up and back axes."""
        v = np.asarray(self.values, dtype=np.float64)
        if self.format in ("quat", "axisangle"):
            w, x, y, z = self.as_quat()
            return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        if self.format == "xyaxes":
            x = v[:3] / np.linalg.norm(v[:3])
            y = v[3:] - (v[3:] @ x) * x
            y = y / np.linalg.norm(y)
            return np.stack([x, y, np.cross(x, y)], axis=1)
        if self.format == "zaxis":
            z = v / np.linalg.norm(v)
            axis = np.cross([0.0, 0.0, 1.0], z)
            s, c = np.linalg.norm(axis), z[2]
            if s < 1e-12:
                return np.eye(3) if c > 0 else np.diag([1.0, -1.0, -1.0])
            k = axis / s
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            return np.eye(3) + s * K + (1 - c) * (K @ K)
        cx, sx, cy, sy, cz, sz = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        return rz @ ry @ rx
