"""Shaders/Skinning/compute.glsl:14-47 restated in numpy binary32, operation for operation in the order k_skin (csrc/kernels_scene.hpp) evaluates it: what idkptSkin is held to,
byte for byte, on all three of its outputs (tests/test_skin_ref.py pins this file to the llvmpipe fixtures; tests/test_gpu_adversarial_skeletons.py holds the device to it).
No library import and no device.

The path of one vertex of the range:
  M[r][c]  = ((w0 * J0[r][c] + w1 * J1[r][c]) + w2 * J2[r][c]) + w3 * J3[r][c]      J_k = joints[joint_offset + JointIndices[k]], weights as given (no normalisation)
  position = ((M[r][0] * p.x + M[r][1] * p.y) + M[r][2] * p.z) + M[r][3] * 1
  v        = decode(word): field / 2047 (z: / 1023), * 2 - 1
  t        = (M[r][0] * v.x + M[r][1] * v.y) + M[r][2] * v.z                         mat3(skinMatrix) * v
  n        = t * (1 / sqrt((t.x * t.x + t.y * t.y) + t.z * t.z))                    normalize: ONE inverse length per vector, its own
  word     = compress(n)
prev_positions[output] = positions[output] BEFORE the store; the uv words of the vertex are copied.  Nothing outside the range is written.

The compression rule for values no field can hold (include/idkpt.h, idkptSkin): u = n * 0.5 + 0.5, x = u * 2047 (z: * 1023), code = rint(fmin(fmax(x, 0), 2047)) — ties to even,
NaN acts as 0 (fmax returns the other operand), -Inf -> 0, +Inf -> the field's all-ones.  Finite n lie in [-1, 1] and are not touched by the clamp."""
import numpy as np

f32 = np.float32
FIELDS = ((0, 2047), (11, 2047), (22, 1023))        # (shift, mask = largest code) of x, y, z


def decompress(words):
    """Compression.glsl DecompressSR11G11B10: (n, 3) float32"""
    w = np.asarray(words, np.uint32)
    out = np.empty(w.shape + (3,), f32)
    for k, (shift, mask) in enumerate(FIELDS):
        out[..., k] = ((w >> np.uint32(shift)) & np.uint32(mask)).astype(f32) / f32(mask) * f32(2.0) - f32(1.0)
    return out


def compress_codes(v):
    """the three codes of CompressSR11G11B10 before the cast, as float32: rint of the clamped u * max (so a test can see .5 ties and the clamp at work through `scaled`)"""
    with np.errstate(all="ignore"):
        v = np.asarray(v, f32)
        u = v * f32(0.5) + f32(0.5)
        scaled = np.stack([u[..., k] * f32(mask) for k, (_, mask) in enumerate(FIELDS)], -1).astype(f32)
        clamped = np.stack([np.fmin(np.fmax(scaled[..., k], f32(0.0)), f32(mask)) for k, (_, mask) in enumerate(FIELDS)], -1).astype(f32)
        return np.rint(clamped).astype(f32), scaled


def compress(v):
    """CompressSR11G11B10 with the rule above: uint32 words"""
    codes, _ = compress_codes(v)
    c = codes.astype(np.uint32)
    return (c[..., 2] << np.uint32(22)) | (c[..., 1] << np.uint32(11)) | c[..., 0]


def blend(un, joints, joint_offset=0):
    """the blended 3 x 4 matrices (n, 3, 4), weights times joint matrices summed in index order"""
    joints = np.asarray(joints, f32).reshape(-1, 3, 4)
    idx = np.asarray(un["JointIndices"], np.int64) + int(joint_offset)
    w = np.asarray(un["JointWeights"], f32)
    with np.errstate(all="ignore"):
        acc = None
        for j in range(4):
            term = (w[:, j, None, None] * joints[idx[:, j]]).astype(f32)
            acc = term if acc is None else (acc + term).astype(f32)
    return acc


def _rows(M, v, w=None):
    with np.errstate(all="ignore"):
        out = []
        for r in range(3):
            a = ((M[:, r, 0] * v[:, 0] + M[:, r, 1] * v[:, 1]).astype(f32) + M[:, r, 2] * v[:, 2]).astype(f32)
            if w is not None:
                a = (a + M[:, r, 3] * f32(w)).astype(f32)
            out.append(a)
        return np.stack(out, 1).astype(f32)


def normalize(t):
    """(normalized, dot, inverse length): v * (1 / sqrt(dot)), dot = (x x + y y) + z z"""
    with np.errstate(all="ignore"):
        d = ((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]).astype(f32) + t[:, 2] * t[:, 2]).astype(f32)
        inv = (f32(1.0) / np.sqrt(d).astype(f32)).astype(f32)
        return (t * inv[:, None]).astype(f32), d, inv


def intermediates(un, joints, joint_offset=0):
    """every stage of the normal / tangent path for the vertices `un` (all of them): dict of arrays — what tests/test_skin_ref.py inspects to see that an edge case is one"""
    M = blend(un, joints, joint_offset)
    out = {"M": M, "position": _rows(M, np.asarray(un["Position"], f32), 1.0)}
    for name in ("Normal", "Tangent"):
        v = decompress(un[name]); t = _rows(M, v); n, d, inv = normalize(t)
        codes, scaled = compress_codes(n)
        out[name] = {"decoded": v, "transformed": t, "dot": d, "inv": inv, "normalized": n, "scaled": scaled, "codes": codes, "word": compress(n)}
    return out


def _skin_numpy(un, joints):
    """the positions alone, for all of `un` with joint offset 0 (tests/test_glref.py, tests/test_glref_full.py and the frame tests use it under this name)"""
    return _rows(blend(un, joints), np.asarray(un["Position"], f32), 1.0)


def skin(unskinned, joints, positions, vertices, input_offset, output_offset, joint_offset, count, prev_positions=None):
    """idkptSkin(input_offset, output_offset, joint_offset, count) on copies: returns (positions (n, 3), prev_positions (n, 3), vertices).  prev_positions: the array as it
    was before the call (None: zeros, what the device holds before the first call)."""
    pos = np.array(positions, f32).reshape(-1, 3).copy()
    prev = np.zeros_like(pos) if prev_positions is None else np.array(prev_positions, f32).reshape(-1, 3).copy()
    verts = np.array(vertices).copy()
    if count == 0:
        return pos, prev, verts
    un = unskinned[input_offset:input_offset + count]
    assert len(un) == count and output_offset + count <= len(pos)
    st = intermediates(un, joints, joint_offset)
    o = slice(output_offset, output_offset + count)
    prev[o] = pos[o]
    pos[o] = st["position"]
    verts["Normal"][o] = st["Normal"]["word"]; verts["Tangent"][o] = st["Tangent"]["word"]
    return pos, prev, verts


def refusal(unskinned, joint_count, vertex_count, input_offset, output_offset, joint_offset, count):
    """why idkptSkin must refuse these arguments (a string), or None: the range against both tables, then every joint index of the range against the joint table, no wrap"""
    if input_offset + count > len(unskinned) or output_offset + count > vertex_count:
        return "range"
    if count and int(joint_offset) + int(np.asarray(unskinned["JointIndices"][input_offset:input_offset + count], np.int64).max()) >= joint_count:
        return "joint"
    return None


def same_positions(a, b):
    """byte equality of float32 arrays, except that two NaNs agree whatever their payload (tests/collide_ref.py same_bits)"""
    a = np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32); b = np.ascontiguousarray(b, f32).reshape(-1).view(np.uint32)
    if a.shape != b.shape:
        return False
    nan_a = (a & 0x7FFFFFFF) > 0x7F800000; nan_b = (b & 0x7FFFFFFF) > 0x7F800000
    return bool(((a == b) | (nan_a & nan_b)).all())


def same_vertices(a, b):
    """vertex records are integers and two uv words that are only ever copied: bytes"""
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
