"""Mesh files of the evaluation path: what NeuS_Trainer.validate_mesh writes through trimesh (NeuS_Trainer.py:287-307) --
binary little-endian PLY, vertices float32 x y z (+ uchar red green blue alpha when coloured), faces ``list uchar int vertex_indices``."""
import struct
import zlib

import numpy as np


def write_ply(path, vertices, triangles, colors=None):
    """vertices (V,3) float, triangles (F,3) int, colors (V,3) float in [0,1] or uint8 (optional)."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(triangles, dtype=np.int32).reshape(-1, 3))
    head = ["ply", "format binary_little_endian 1.0", "comment color-neus_amd", f"element vertex {v.shape[0]}",
            "property float x", "property float y", "property float z"]
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = np.asarray(colors)
        if c.dtype != np.uint8:
            c = (np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)     # NeuS_Trainer.py:292 (colors * 255).astype(np.uint8)
        c = c.reshape(-1, 3)
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
        vdt += [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(v.shape[0], dtype=vdt)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vrec["red"], vrec["green"], vrec["blue"], vrec["alpha"] = c[:, 0], c[:, 1], c[:, 2], 255
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"], frec["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """Reader for the files write_ply produces (tests / round trips): (vertices, triangles, colors or None)."""
    with open(path, "rb") as fh:
        lines = []
        while True:
            ln = fh.readline().decode("ascii").strip()
            lines.append(ln)
            if ln == "end_header":
                break
        nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
        nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
        colored = any(l.startswith("property uchar red") for l in lines)
        vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")] if colored else [])
        v = np.frombuffer(fh.read(nv * np.dtype(vdt).itemsize), dtype=vdt)
        f = np.frombuffer(fh.read(nf * 13), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    verts = np.stack([v["x"], v["y"], v["z"]], -1)
    cols = np.stack([v["red"], v["green"], v["blue"]], -1) if colored else None
    return verts, f["i"].copy(), cols


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_vertices(path):
    """Vertex positions of an ASCII or binary-little-endian PLY file as a float32 (V, 3) array, driven by the header: the ``vertex`` element may
    carry any scalar properties of the standard types besides x / y / z (normals, colours, ... are skipped) and need not be followed by a face
    element -- ground-truth clouds come from other writers than write_ply.  Elements in front of the vertex element must have scalar
    properties only (their size is then known without parsing them)."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []          # elements: [name, count, [(property name, numpy type)]]
        while True:
            raw = fh.readline()
            if not raw:
                raise ValueError(f"{path}: PLY header without end_header")
            tok = raw.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "end_header":
                break
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: property in front of the first element")
                if tok[1] == "list":
                    elements[-1][2].append((tok[-1], None))
                elif tok[1] in _PLY_TYPES:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
                else:
                    raise ValueError(f"{path}: unknown PLY property type '{tok[1]}'")
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: PLY format '{fmt}' is not supported (ascii and binary_little_endian are)")
        for name, count, props in elements:
            if any(t is None for _, t in props):
                raise ValueError(f"{path}: element '{name}' with a list property in front of / as the vertex element")
            if name != "vertex":
                if fmt == "ascii":        # one line per entry
                    for _ in range(count):
                        fh.readline()
                else:
                    fh.seek(count * sum(np.dtype(t).itemsize for _, t in props), 1)
                continue
            names = [n for n, _ in props]
            if not all(c in names for c in "xyz"):
                raise ValueError(f"{path}: the vertex element has no x / y / z")
            if fmt == "ascii":
                rows = [fh.readline().split() for _ in range(count)]
                if any(len(r) < len(props) for r in rows):
                    raise ValueError(f"{path}: short vertex line")
                cols = [names.index(c) for c in "xyz"]
                return np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(np.float32).reshape(count, 3)
            dt = np.dtype([(n, "<" + t) for n, t in props])
            buf = fh.read(count * dt.itemsize)
            if len(buf) != count * dt.itemsize:
                raise ValueError(f"{path}: truncated vertex data")
            v = np.frombuffer(buf, dtype=dt)
            return np.stack([v["x"], v["y"], v["z"]], -1).astype(np.float32).reshape(count, 3)
    raise ValueError(f"{path}: no vertex element")


def write_png(path, image_uint8):
    """An 8-bit PNG of a ``[H, W, 3]`` (RGB, written as given) or ``[H, W]`` (grey) uint8 array or tensor: what the reference saves with
    imageio (NeuS_Trainer.py:274), with zlib and struct from the standard library only.  Filter type 0 on every row, one IDAT chunk."""
    if hasattr(image_uint8, "detach"):
        image_uint8 = image_uint8.detach().cpu().numpy()
    img = np.ascontiguousarray(image_uint8)
    if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_png: expected a uint8 [H, W, 3] or [H, W] image, got {img.dtype} {img.shape}")
    h, w = img.shape[0], img.shape[1]
    rows = np.zeros((h, 1 + img[0].size), dtype=np.uint8)      # a filter-type byte (0: none) in front of every row
    rows[:, 1:] = img.reshape(h, -1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
