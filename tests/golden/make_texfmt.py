"""Mints tests/golden/texfmt/bc7_blocks.npz: BC7 blocks of every (mode, selector) pair and what an independent decoder — Pillow's compiled BCn decoder, through an in-memory
DX10 DDS of DXGI format 98 (BC7_UNORM) — makes of them.  CPU only; needs Pillow (no test imports it unconditionally: tests/test_texfmt_ref.py re-mints and compares when it is there).

  blocks  uint8 [n, 16]        the blocks
  texels  uint8 [n, 4, 4, 4]   [block, y, x, RGBA]

For every pair, four blocks with the mode bits and the selector set and all remaining bits random (fixed seed): mode 0 x 16 partitions, modes 1, 2, 3, 7 x 64 partitions,
mode 4 x 4 rotations x 2 index selections, mode 5 x 4 rotations, mode 6: 285 pairs, 1 140 blocks.  Then eight blocks with byte 0 == 0 (reserved): their texels are written as
zeros HERE, as ARB_texture_compression_bptc defines them — Pillow 12.2 returns (0, 0, 0, 255) for such a block, alpha opaque, which is not what the specification says.

Usage: python tests/golden/make_texfmt.py   (rewrites the file in place)"""
import io
import os
import struct
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "texfmt", "bc7_blocks.npz")
SEED, PER_PAIR, RESERVED = 20260, 4, 8


def pairs():
    """(mode, selector, first bit of the selector field, its width) of every pair, in fixture order."""
    out = [(0, p, 1, 4) for p in range(16)]
    for m in (1, 2, 3, 7):
        out += [(m, p, m + 1, 6) for p in range(64)]
    out += [(4, s, 5, 3) for s in range(8)]          # rotation (2 bits) | index selection << 2
    out += [(5, r, 6, 2) for r in range(4)]
    out += [(6, 0, 7, 0)]
    return out


def make_blocks():
    rng = np.random.default_rng(SEED)
    blocks = []
    for (mode, selv, pos, width) in pairs():
        for _ in range(PER_PAIR):
            v = int.from_bytes(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
            v &= ~((1 << (pos + width)) - 1)           # mode bits and selector cleared ...
            v |= (1 << mode) | (selv << pos)           # ... and set
            blocks.append(np.frombuffer(v.to_bytes(16, "little"), np.uint8))
    for _ in range(RESERVED):
        b = rng.integers(0, 256, 16, dtype=np.uint8); b[0] = 0
        blocks.append(b)
    return np.stack(blocks)


def selector_of(block):
    """(mode, selector) parsed from a block; (8, 0) for a reserved one."""
    v = int.from_bytes(bytes(block), "little")
    if block[0] == 0:
        return (8, 0)
    mode = (int(block[0]) & -int(block[0])).bit_length() - 1
    pos, width = {0: (1, 4), 1: (2, 6), 2: (3, 6), 3: (4, 6), 4: (5, 3), 5: (6, 2), 6: (7, 0), 7: (8, 6)}[mode]
    return (mode, (v >> pos) & ((1 << width) - 1))


def dds_dx10(dxgi_format, width, height, payload):
    """A DX10-header DDS file around `payload`."""
    hdr = struct.pack("<4s7I44x", b"DDS ", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, height, width, len(payload), 0, 1)
    hdr += struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    return hdr + struct.pack("<5I", dxgi_format, 3, 0, 1, 0) + payload


def pillow_decode_bc7(blocks):
    from PIL import Image
    n = len(blocks)
    im = Image.open(io.BytesIO(dds_dx10(98, 4 * n, 4, np.ascontiguousarray(blocks, np.uint8).tobytes()))); im.load()
    a = np.asarray(im.convert("RGBA"))               # one row of n blocks
    return np.ascontiguousarray(a.reshape(4, n, 4, 4).transpose(1, 0, 2, 3))


def mint():
    blocks = make_blocks()
    texels = pillow_decode_bc7(blocks)
    texels[blocks[:, 0] == 0] = 0                      # reserved blocks: the specification's zeros (see above)
    return blocks, texels


if __name__ == "__main__":
    blocks, texels = mint()
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, blocks=blocks, texels=texels)
    print(PATH, blocks.shape, texels.shape, os.path.getsize(PATH), "bytes")
