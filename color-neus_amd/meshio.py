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


def _ply_header(fh, path):
    """(format, [[element name, count, [(property name, numpy type -- or (count type, item type) for a list property)]]]) of an open PLY file,
    which is left at the first byte behind ``end_header``."""
    if fh.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
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
                if len(tok) < 5 or tok[2] not in _PLY_TYPES or tok[3] not in _PLY_TYPES:
                    raise ValueError(f"{path}: malformed PLY list property")
                elements[-1][2].append((tok[-1], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            elif tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            else:
                raise ValueError(f"{path}: unknown PLY property type '{tok[1]}'")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format '{fmt}' is not supported (ascii and binary_little_endian are)")
    return fmt, elements


def _ply_vertex_rows(fh, path, fmt, count, props):
    """The x / y / z of a vertex element with scalar properties, the file positioned at its first entry: float32 (count, 3)."""
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


def _ply_skip(fh, fmt, count, props):
    """Step over an element with scalar properties only."""
    if fmt == "ascii":        # one line per entry
        for _ in range(count):
            fh.readline()
    else:
        fh.seek(count * sum(np.dtype(t).itemsize for _, t in props), 1)


def read_ply_vertices(path):
    """Vertex positions of an ASCII or binary-little-endian PLY file as a float32 (V, 3) array, driven by the header: the ``vertex`` element may
    carry any scalar properties of the standard types besides x / y / z (normals, colours, ... are skipped) and need not be followed by a face
    element -- ground-truth clouds come from other writers than write_ply.  Elements in front of the vertex element must have scalar
    properties only (their size is then known without parsing them)."""
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh, path)
        for name, count, props in elements:
            if any(isinstance(t, tuple) for _, t in props):
                raise ValueError(f"{path}: element '{name}' with a list property in front of / as the vertex element")
            if name != "vertex":
                _ply_skip(fh, fmt, count, props)
                continue
            return _ply_vertex_rows(fh, path, fmt, count, props)
    raise ValueError(f"{path}: no vertex element")


def read_ply_mesh(path):
    """``(vertices float32 (V, 3), triangles int32 (F, 3) or None)`` of an ASCII or binary-little-endian PLY file, driven by the header like
    ``read_ply_vertices``: the vertex element may carry further scalar properties; the ``face`` element -- None is returned for the triangles
    when the file has none -- must hold a ``vertex_indices`` or ``vertex_index`` list of exactly three entries per face and may carry scalar
    properties besides it.  A face with another number of corners, a face element without that list or with a second list, and a list
    property in any other element raise ValueError.  Elements behind the face element are not read."""
    verts = tris = None
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh, path)
        for name, count, props in elements:
            lists = [(i, n) for i, (n, t) in enumerate(props) if isinstance(t, tuple)]
            if name == "vertex":
                if lists:
                    raise ValueError(f"{path}: the vertex element has a list property")
                verts = _ply_vertex_rows(fh, path, fmt, count, props)
            elif name == "face":
                if len(lists) != 1 or lists[0][1] not in ("vertex_indices", "vertex_index"):
                    raise ValueError(f"{path}: the face element needs exactly one list property, vertex_indices or vertex_index")
                at = lists[0][0]
                ct, it = props[at][1]
                if it[0] == "f":
                    raise ValueError(f"{path}: vertex indices of a float type")
                if fmt == "ascii":
                    rows = [fh.readline().split() for _ in range(count)]
                    if any(len(r) <= at or int(r[at]) != 3 or len(r) < len(props) + 3 for r in rows):
                        raise ValueError(f"{path}: a face that is not a triangle (or a short face line)")
                    tris = np.array([[int(x) for x in r[at + 1:at + 4]] for r in rows], dtype=np.int64).reshape(count, 3)
                else:
                    dt = np.dtype([(n, "<" + t) if not isinstance(t, tuple) else (n, [("n", "<" + ct), ("i", "<" + it, (3,))]) for n, t in props])
                    buf = fh.read(count * dt.itemsize)          # (every record has this size iff every face is a triangle: checked below)
                    if len(buf) != count * dt.itemsize:
                        raise ValueError(f"{path}: a face that is not a triangle (or truncated face data)")
                    f = np.frombuffer(buf, dtype=dt)[props[at][0]]
                    if count and bool((f["n"] != 3).any()):
                        raise ValueError(f"{path}: a face that is not a triangle")
                    tris = f["i"].astype(np.int64).reshape(count, 3)
                if tris.size and (tris.min() < -2 ** 31 or tris.max() > 2 ** 31 - 1):
                    raise ValueError(f"{path}: a vertex index that does not fit int32")
                tris = tris.astype(np.int32)
            else:
                if lists:
                    raise ValueError(f"{path}: element '{name}' with a list property")
                _ply_skip(fh, fmt, count, props)
            if verts is not None and tris is not None:
                break
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return verts, tris


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
