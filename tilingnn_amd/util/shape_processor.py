"""Silhouette files (the reference's util/shape_processor.py: `load_polygons`).

Format: one ring per line, vertices separated by commas, each vertex "x y".  Line 0 is the exterior, every further line a
hole.  SVG parsing (`getSVGShapeAsNp`) is not mirrored.
"""
import numpy as np


def _parse_ring(line: str) -> np.ndarray:
    pts = []
    for word in line.split(","):
        parts = word.split(" ")
        pts.append([float(parts[0]), float(parts[1])])
    return np.array(pts)


def load_polygons(filename):
    """(exterior [n, 2] float64, [hole [m, 2] float64, ...])."""
    with open(filename) as f:
        lines = f.readlines()
    return _parse_ring(lines[0]), [_parse_ring(line) for line in lines[1:]]
