"""Loaders for the committed golden fixtures (tests/golden/*.npz, made by generate_golden.py)."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_labyrinth_graph():
    """The real data/labyrinth/complete_graph_ring9 graph, expanded to the arrays
    BrickLayout.get_data_as_torch_tensor would produce (float64 / int64 numpy)."""
    z = np.load(os.path.join(GOLDEN, "labyrinth_ring9_graph.npz"))
    n, tc = z["node_type"].shape[0], int(z["tile_count"])
    x = np.zeros((n, tc + 1))
    x[np.arange(n), z["node_type"]] = 1.0
    x[:, -1] = z["node_area"]
    adj_attr = z["adj_rows"][z["adj_type"]]
    col_attr = np.zeros((z["col"].shape[1], adj_attr.shape[1]))
    col_attr[:, 0] = z["col_areas"][z["col_area_type"]]
    return dict(x=x, adj=z["adj"].astype(np.int64), adj_attr=adj_attr, col=z["col"].astype(np.int64),
                col_attr=col_attr, tile_count=tc, adj_type=z["adj_type"].astype(np.int64))


def graph_tensors(g, dtype=torch.float32, device="cpu"):
    return (torch.from_numpy(np.asarray(g["x"])).to(dtype).to(device),
            torch.from_numpy(np.asarray(g["adj"]).astype(np.int64)).to(device),
            torch.from_numpy(np.asarray(g["adj_attr"])).to(dtype).to(device),
            torch.from_numpy(np.asarray(g["col"]).astype(np.int64)).to(device),
            torch.from_numpy(np.asarray(g["col_attr"])).to(dtype).to(device))


class _NpzParts(dict):
    """The members of a fixture stored in parts, merged; `files` as np.load's NpzFile has it."""

    @property
    def files(self):
        return list(self)


def part_paths(name):
    stem = os.path.join(GOLDEN, name[:-len(".npz")])
    return sorted(glob.glob(stem + ".part*.npz"), key=lambda p: int(p[len(stem) + len(".part"):-len(".npz")]))


def save_npz_parts(name, arrays, limit=900 * 1024):
    """np.savez_compressed of `arrays` as contiguous runs of its members of at most `limit` bytes each, <stem>.part<k>.npz (no
    committed file may exceed 1 MiB); load_npz(name) merges them again."""
    for p in part_paths(name):
        os.remove(p)
    runs, size = [[]], 0
    for key, a in arrays.items():
        cost = np.asarray(a).nbytes + 512 + 2 * len(key)          # (+ the member's .npy header and zip directory entries)
        if runs[-1] and size + cost > limit:
            runs.append([])
            size = 0
        runs[-1].append(key)
        size += cost
    paths = []
    for k, run in enumerate(runs):
        paths.append(os.path.join(GOLDEN, f"{name[:-len('.npz')]}.part{k}.npz"))
        np.savez_compressed(paths[-1], **{key: arrays[key] for key in run})
        assert os.path.getsize(paths[-1]) < 2 ** 20, (paths[-1], run)
    return paths


def load_npz(name):
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path)
    parts = part_paths(name)
    if not parts:
        raise FileNotFoundError(path)
    merged = _NpzParts()
    for p in parts:
        with np.load(p) as z:
            merged.update((k, z[k]) for k in z.files)
    return merged
