"""Minimal PLY reader for point clouds (replaces the Open3D read used by the
reference at lib/utils.py:48 and scripts/pairwise_demo.py:75).  Supports
binary_little_endian / binary_big_endian / ascii vertex elements; returns the
x, y, z properties as float32 [N, 3] (Open3D widens them to float64), and with
read_ply_colors the red, green, blue properties beside them."""
import numpy as np

_TYPES = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4",
          "double": "f8", "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4",
          "uint32": "u4", "float32": "f4", "float64": "f8"}


def _read_vertices(path):
    """-> (the vertex element's property names and type codes, column(name) -> its values [N])"""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, props, count, in_vertex, pre = None, [], 0, False, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
                elif count == 0:
                    pre.append((tok[1], int(tok[2])))
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("list properties in the vertex element are not supported")
                props.append((tok[2], _TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if pre:
            raise ValueError("elements before 'vertex' are not supported")
        if fmt == "ascii":
            data = np.loadtxt(f, max_rows=count, ndmin=2)
            names = [p[0] for p in props]
            return dict(props), lambda name: data[:, names.index(name)]
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(n, end + t) for n, t in props])
        arr = np.frombuffer(f.read(dt.itemsize * count), dtype=dt, count=count)
        return dict(props), lambda name: arr[name]


def read_ply_xyz(path):
    _, column = _read_vertices(path)
    return np.stack([column(a) for a in "xyz"], 1).astype(np.float32)


def read_ply_colors(path):
    """-> (xyz float32 [N,3], colors float64 [N,3] in [0, 1], or None when the file has no red / green / blue).  The
    three properties are picked by name: uchar values are divided by 255, float values taken as they are (Open3D's
    convention for float colours), any other integer type by its own largest value."""
    props, column = _read_vertices(path)
    xyz = np.stack([column(a) for a in "xyz"], 1).astype(np.float32)
    rgb = ("red", "green", "blue")
    if not all(c in props for c in rgb):
        return xyz, None
    cols = []
    for c in rgb:
        v = np.asarray(column(c), dtype=np.float64)
        if props[c][0] in "iu":
            v = v / float(np.iinfo(np.dtype(props[c])).max)
        cols.append(v)
    return xyz, np.stack(cols, 1)


def write_ply_xyz(path, xyz):
    xyz = np.asarray(xyz, dtype="<f4")
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n" % len(xyz)).encode())
        f.write(xyz.tobytes())


def write_ply(path, xyz, normals=None, colors=None):
    """Points [N,3] and, when given, their normals [N,3] as little-endian float properties x y z (nx ny nz) and their
    colours [N,3] (float in [0, 1], or uint8) as uchar red green blue; the file reads back through read_ply_xyz and
    read_ply_colors, which pick their properties by name."""
    xyz = np.asarray(xyz, dtype="<f4").reshape(-1, 3)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8:
            colors = np.clip(np.rint(np.asarray(colors, dtype=np.float64) * 255.0), 0.0, 255.0).astype(np.uint8)
        colors = colors.reshape(-1, 3)
        if len(colors) != len(xyz):
            raise ValueError("write_ply: %d colours for %d points" % (len(colors), len(xyz)))
    cols, names = [xyz], ["x", "y", "z"]
    if normals is not None:
        normals = np.asarray(normals, dtype="<f4").reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError("write_ply: %d normals for %d points" % (len(normals), len(xyz)))
        cols, names = [xyz, normals], names + ["nx", "ny", "nz"]
    floats = np.ascontiguousarray(np.concatenate(cols, 1))
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s%send_header\n"
                 % (len(xyz), "".join("property float %s\n" % n for n in names),
                    "" if colors is None else "".join("property uchar %s\n" % n for n in ("red", "green", "blue"))
                    )).encode())
        if colors is None:
            f.write(floats.tobytes())
        else:
            rows = np.empty(len(xyz), dtype=[("f", "<f4", (floats.shape[1],)), ("c", "u1", (3,))])
            rows["f"], rows["c"] = floats, colors
            f.write(rows.tobytes())

