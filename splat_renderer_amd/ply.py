"""Trained 3D Gaussian splatting scenes from PLY files (footprint="ellipsoid"; an extension, no reference counterpart).

load_gaussian_ply reads the binary_little_endian vertex layout that 3D Gaussian splatting writes — x y z, f_dc_0..2,
f_rest_0..N, opacity, scale_0..2, rot_0..3 (other float properties such as nx ny nz are skipped) — with NumPy alone, and
applies the activations the renderer expects: scale = exp(scale_k), opacity = sigmoid(opacity), the quaternion as
(w, x, y, z) = (rot_0, rot_1, rot_2, rot_3).  The file stores the higher SH coefficients channel-major (all of red, then
green, then blue); they are returned basis-major, sh[i, k, c], with the DC term as k = 0.  The degree follows from the
number of f_rest properties: 0, 9, 24 or 45 for degrees 0-3.

load_point_ply reads what a fit starts from instead: a coloured point cloud, x y z and red green blue per vertex.

save_gaussian_ply is its exact inverse: the same file 3D Gaussian splatting writes (x y z, zero nx ny nz, f_dc, channel-major
f_rest, opacity as a logit, log scales, rot), from the arrays load_gaussian_ply returns.

load_surfel_ply and save_surfel_ply are the same pair for 2D Gaussian surfels (2DGS's files; SurfelFit.save_ply): the same
properties in the same order with scale_0 and scale_1 only.  Each loader refuses the other's file.

save_mesh_ply writes a triangle mesh (TsdfVolume.extract_mesh's, GaussianFit.extract_mesh's): vertex and face elements, uchar colours.
"""
import numpy as np

from ._lib import SplatError

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_REST_TO_DEGREE = {0: 0, 9: 1, 24: 2, 45: 3}


def _bad(path, why):
    return SplatError(-1, f"{path}: not a 3D Gaussian splatting PLY file: {why}")


def _bad_points(path, why):
    return SplatError(-1, f"{path}: not a point-cloud PLY file: {why}")


def _read_vertex_header(f, path, bad):
    """The header of a binary_little_endian PLY whose vertex element is the first and only element with data, f left at the
    first vertex: (n, [(property name, NumPy type), ...]).  bad(path, why) makes the error."""
    if f.readline().rstrip(b"\r\n") != b"ply":
        raise bad(path, "no 'ply' magic line")
    fmt, n, props, in_vertex, other = None, None, [], False, False
    while True:
        line = f.readline()
        if not line:
            raise bad(path, "the header has no end_header line")
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else None
        elif words[0] == "element":
            if len(words) != 3:
                raise bad(path, f"malformed element line {line!r}")
            in_vertex = words[1] == "vertex"
            if in_vertex:
                if n is not None or other:
                    raise bad(path, "the vertex element must be the first and only element with data")
                n = int(words[2])
            elif int(words[2]) > 0:
                other = True
        elif words[0] == "property":
            if len(words) != 3 or words[1] == "list":
                raise bad(path, f"unsupported property {line!r} (list properties are not vertex attributes)")
            if words[1] not in _PLY_TYPES:
                raise bad(path, f"unknown property type {words[1]!r}")
            if in_vertex:
                props.append((words[2], "<" + _PLY_TYPES[words[1]]))
    if fmt != "binary_little_endian":
        raise bad(path, f"format {fmt!r}; only binary_little_endian is read")
    if n is None:
        raise bad(path, "no vertex element")
    names = [p[0] for p in props]
    if len(set(names)) != len(names):
        raise bad(path, "a property name repeats")
    return n, props


def _read_vertices(f, path, bad, n, props):
    dtype = np.dtype(props)
    raw = f.read(n * dtype.itemsize)
    if len(raw) != n * dtype.itemsize:
        raise bad(path, f"the file ends after {len(raw) // dtype.itemsize} of {n} vertices")
    return np.frombuffer(raw, dtype=dtype, count=n)


def load_point_ply(path):
    """A coloured point cloud, what structure from motion leaves (COLMAP's points3D.ply): (xyz float32 (n, 3), rgb float32 (n, 3)
    in [0, 1]) from a binary_little_endian PLY whose vertices carry x y z as float or double and red green blue as uchar.  Other
    properties (normals, errors, track lengths) are skipped.  GaussianFit.from_points takes the pair."""
    with open(path, "rb") as f:
        n, props = _read_vertex_header(f, path, _bad_points)
        types = dict(props)
        missing = [k for k in ("x", "y", "z", "red", "green", "blue") if k not in types]
        if missing:
            raise _bad_points(path, f"missing properties {missing}")
        for k in ("x", "y", "z"):
            if types[k] not in ("<f4", "<f8"):
                raise _bad_points(path, f"property {k} is {types[k]!r}; float or double is expected")
        for k in ("red", "green", "blue"):
            if types[k] != "<u1":
                raise _bad_points(path, f"property {k} is {types[k]!r}; uchar is expected")
        v = _read_vertices(f, path, _bad_points, n, props)
    xyz = np.ascontiguousarray(np.stack([v[k].astype(np.float32) for k in ("x", "y", "z")], axis=1), dtype=np.float32).reshape(n, 3)
    rgb = np.ascontiguousarray(np.stack([v[k].astype(np.float32) / np.float32(255.0) for k in ("red", "green", "blue")], axis=1),
                               dtype=np.float32).reshape(n, 3)
    return xyz, rgb


def _bad_surfels(path, why):
    return SplatError(-1, f"{path}: not a 2D Gaussian splatting PLY file: {why}")


def load_gaussian_ply(path):
    """Returns a dict of float32 arrays: positions (n, 3), scales (n, 3), rotations (n, 4) as (w, x, y, z), opacity (n,),
    sh (n, (degree + 1)^2, 3), and the int degree.  Pass them to GaussianCloud.fromArrays(device, positions, scales,
    rotations, opacity=opacity, sh=sh)."""
    return _load_splat_ply(path, 3, _bad)


def load_surfel_ply(path):
    """A 2D Gaussian splatting file (2DGS's layout: 3DGS's with scale_0 and scale_1 only): load_gaussian_ply's dict with scales
    (n, 2), the standard deviations along the surfel's two tangent axes, as autograd.render_surfels and SurfelFit take them.  A
    file with a scale_2 property is a 3D Gaussian splatting file and is refused: load_gaussian_ply reads it."""
    return _load_splat_ply(path, 2, _bad_surfels)


def _load_splat_ply(path, n_scales, bad):
    scale_keys = [f"scale_{j}" for j in range(n_scales)]
    with open(path, "rb") as f:
        n, props = _read_vertex_header(f, path, bad)
        names = [p[0] for p in props]
        need = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"] + scale_keys + ["rot_0", "rot_1", "rot_2", "rot_3"]
        missing = [k for k in need if k not in names]
        if missing:
            raise bad(path, f"missing properties {missing}")
        if n_scales == 2 and "scale_2" in names:
            raise bad(path, "it has a scale_2 property: a 3D Gaussian splatting file, which load_gaussian_ply reads")
        rest = sorted((k for k in names if k.startswith("f_rest_")), key=lambda k: int(k[len("f_rest_"):]))
        if len(rest) not in _REST_TO_DEGREE or rest != [f"f_rest_{j}" for j in range(len(rest))]:
            raise bad(path, f"{len(rest)} f_rest properties; 0, 9, 24 or 45 (f_rest_0 ... in order) are expected")
        v = _read_vertices(f, path, bad, n, props)

    def cols(keys):
        return np.stack([v[k].astype(np.float32) for k in keys], axis=1) if keys else np.zeros((n, 0), np.float32)

    degree = _REST_TO_DEGREE[len(rest)]
    nb = (degree + 1) ** 2
    dc = cols(["f_dc_0", "f_dc_1", "f_dc_2"])
    # channel-major f_rest: f_rest_{c * (nb - 1) + (k - 1)} is channel c of basis k
    hi = cols(rest).reshape(n, 3, nb - 1).transpose(0, 2, 1)
    sh = np.ascontiguousarray(np.concatenate([dc[:, None, :], hi], axis=1), dtype=np.float32)
    op = cols(["opacity"])[:, 0]
    return {
        "positions": cols(["x", "y", "z"]),
        # (both activations in float64, rounded once: the same arrays on every host, whatever its NumPy's float32 exp)
        "scales": np.exp(cols(scale_keys).astype(np.float64)).astype(np.float32),
        "rotations": cols(["rot_0", "rot_1", "rot_2", "rot_3"]),
        "opacity": (1.0 / (1.0 + np.exp(-op.astype(np.float64)))).astype(np.float32),
        "sh": sh,
        "degree": degree,
    }


def save_mesh_ply(path, vertices, triangles, colors=None):
    """A triangle mesh as a binary_little_endian PLY any mesh viewer reads: element vertex with float x y z (and, with colors,
    uchar red green blue: round(255 c) clamped to [0, 255]), element face with `property list uchar int vertex_indices`.
    vertices (V, 3) float32, triangles (T, 3) integers in [0, V), colors (V, 3) in [0, 1] or None: NumPy arrays or anything
    np.asarray takes (device tensors are downloaded by the caller: TsdfVolume.extract_mesh's results want .cpu() first).
    Positions and indices are stored bit for bit."""
    v = np.asarray(vertices, np.float32)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise SplatError(-1, "save_mesh_ply: vertices (V, 3) floats and triangles (T, 3) integers are expected")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= v.shape[0]):
        raise SplatError(-1, f"save_mesh_ply: a triangle names a vertex outside [0, {v.shape[0]})")
    fields = [("xyz", "<f4", 3)]
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {v.shape[0]}\n" + "property float x\nproperty float y\nproperty float z\n"
    if colors is not None:
        c = np.asarray(colors, np.float32)
        if c.shape != v.shape:
            raise SplatError(-1, f"save_mesh_ply: colors must have shape {v.shape}, not {c.shape}")
        fields.append(("rgb", "u1", 3))
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += f"element face {t.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n"
    vt = np.zeros(v.shape[0], np.dtype(fields))
    vt["xyz"] = v
    if colors is not None:
        with np.errstate(invalid="ignore"):
            vt["rgb"] = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
    ft = np.zeros(t.shape[0], np.dtype([("n", "u1"), ("idx", "<i4", 3)]))
    ft["n"] = 3
    ft["idx"] = t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vt.tobytes())
        f.write(ft.tobytes())


def save_gaussian_ply(path, positions, scales, rotations, opacity, sh, log_scales=None, opacity_logits=None):
    """Writes the cloud as 3D Gaussian splatting does (binary_little_endian float properties in its order: x y z, nx ny nz = 0,
    f_dc_0..2, f_rest_* channel-major, opacity, scale_0..2, rot_0..3): load_gaussian_ply's inverse.  positions (n, 3), scales
    (n, 3) > 0, rotations (n, 4) as (w, x, y, z), opacity (n,) in (0, 1), sh (n, (degree + 1)^2, 3) or (n, 3 (degree + 1)^2)
    basis-major.  The file stores log(scales) and logit(opacity), formed in float64 and rounded once.  A caller that holds the
    raw parameters passes them as log_scales / opacity_logits (scales / opacity may then be None): they are stored as they are,
    bit for bit.  Positions, rotations and SH are stored bit for bit."""
    _save_splat_ply("save_gaussian_ply", 3, path, positions, scales, rotations, opacity, sh, log_scales, opacity_logits)


def save_surfel_ply(path, positions, scales, rotations, opacity, sh, log_scales=None, opacity_logits=None):
    """Writes 2D Gaussian surfels as 2DGS does: save_gaussian_ply's properties in its order with scale_0 and scale_1 only;
    load_surfel_ply's inverse.  scales (n, 2) > 0; everything else, the raw planes (log_scales (n, 2)) included, as
    save_gaussian_ply takes it."""
    _save_splat_ply("save_surfel_ply", 2, path, positions, scales, rotations, opacity, sh, log_scales, opacity_logits)


def _save_splat_ply(who, n_scales, path, positions, scales, rotations, opacity, sh, log_scales, opacity_logits):
    pos = np.asarray(positions, np.float32)
    n = pos.shape[0]
    rot = np.asarray(rotations, np.float32)
    coef = np.asarray(sh, np.float32).reshape(n, -1, 3)
    nb = coef.shape[1]
    degree = {1: 0, 4: 1, 9: 2, 16: 3}.get(nb)
    if degree is None:
        raise SplatError(-1, f"{who}: sh must hold 3 (degree + 1)^2 floats per splat, degree 0-3, not {3 * nb}")
    with np.errstate(all="ignore"):
        ls = (np.asarray(log_scales, np.float32) if log_scales is not None
              else np.log(np.asarray(scales, np.float32).astype(np.float64)).astype(np.float32))
        if opacity_logits is not None:
            ol = np.asarray(opacity_logits, np.float32).reshape(-1)
        else:
            o = np.asarray(opacity, np.float32).reshape(-1).astype(np.float64)
            ol = (np.log(o) - np.log1p(-o)).astype(np.float32)
    if pos.shape != (n, 3) or ls.shape != (n, n_scales) or rot.shape != (n, 4) or ol.shape != (n,):
        raise SplatError(-1, f"{who}: positions (n, 3), scales (n, {n_scales}), rotations (n, 4) and opacity (n,) are expected")
    rest = coef[:, 1:, :].transpose(0, 2, 1).reshape(n, 3 * (nb - 1))  # channel-major: f_rest_{c (nb - 1) + (k - 1)}
    names = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{j}" for j in range(rest.shape[1])]
             + ["opacity"] + [f"scale_{j}" for j in range(n_scales)] + ["rot_0", "rot_1", "rot_2", "rot_3"])
    table = np.concatenate([pos, np.zeros((n, 3), np.float32), coef[:, 0, :], rest, ol[:, None], ls, rot], axis=1).astype("<f4")
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property float {k}\n" for k in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(table).tobytes())
