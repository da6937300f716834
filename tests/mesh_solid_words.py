"""A word-level model of the solid fill's merge (k_ms_merge in sdf_tools_amd/csrc/sdfgpu_mesh_solid.hip), numpy
only: from the toggle counts of ONE mesh (mesh_solid_restated.toggles_of over every column) to that mesh's parity bits on the unpadded
bit field, by the steps the kernel takes:

  per column wz = ceil(nz / 32) padded toggle words (a crossing above the last centre toggles nothing)
  the prefix XOR within a word (five shift-XOR steps)
  the carry across the words of a chunk of 64 (the parity of the words' top bits below this word) and across chunks
  the tail mask on the last word
  the shift left by sh = (b0 & 31), b0 = (x ny + y) nz, taking the high part of the word before (across chunks: the last of the chunk before)
  the spill of the last word's high part into word (b0 >> 5) + wz

It is a description of the algorithm and is not derived from the kernel's output.  Its one use (test_mesh_solid_cpu.py) is to show,
without a GPU, that the scenes of mesh_solid_cases.stack_scene tell each of the FAULTS below from the truth: `fault` leaves one step out."""
import numpy as np

CHUNK = 64
FAULTS = ("no-chunk-carry", "no-word-carry", "no-tail-mask", "no-spill-word", "no-prev-across-chunks")


def toggle_words(toggles):
    """[nx, ny, nz + 1] counts -> (uint32 [nx ny, wz] toggle words, nz)"""
    nx, ny, nz = toggles.shape[0], toggles.shape[1], toggles.shape[2] - 1
    wz = (nz + 31) // 32
    bit = np.zeros((nx * ny, wz * 32), np.uint64)
    bit[:, :nz] = (toggles[:, :, :nz].reshape(nx * ny, nz) & 1).astype(np.uint64)
    return (bit.reshape(nx * ny, wz, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32), nz


def parity_bits(toggles, fault=None):
    """the parity bits of one mesh on the unpadded field: uint32 [ceil(nx ny nz / 32)]"""
    if fault is not None and fault not in FAULTS:
        raise KeyError(fault)
    words, nz = toggle_words(np.asarray(toggles))
    columns, wz = words.shape
    field = (columns * nz + 31) // 32
    bits = np.zeros(field + 2, np.uint32)                                    # (two spare words: a fault may write past the field)
    b0 = np.arange(columns, dtype=np.int64) * nz
    sh = (b0 & 31).astype(np.uint32)
    back = np.where(sh > 0, 32 - sh, 0).astype(np.uint32)                    # (a shift by 32 is not defined: masked below)
    tail = np.uint32((1 << (nz & 31)) - 1 if nz & 31 else 0xFFFFFFFF)
    carry = np.zeros(columns, np.uint32)                                     # the parity below this chunk
    before = np.zeros(columns, np.uint32)                                    # the last word of the chunk before
    for first in range(0, wz, CHUNK):
        below = np.zeros(columns, np.uint32)                                 # the parity of the top bits of this chunk's words so far
        prev = np.zeros(columns, np.uint32) if (fault == "no-prev-across-chunks" and first) else before
        for j in range(first, min(first + CHUNK, wz)):
            w = words[:, j].copy()
            for step in (1, 2, 4, 8, 16):
                w ^= w << np.uint32(step)
            top = w >> np.uint32(31)
            flip = carry if fault == "no-word-carry" else below ^ carry
            w = np.where(flip == 1, ~w, w)
            below ^= top
            if j == wz - 1 and fault != "no-tail-mask":
                w &= tail
            out = np.where(sh > 0, (w << sh) | (prev >> back), w)
            np.bitwise_or.at(bits, (b0 >> 5) + j, out)
            if j == wz - 1 and fault != "no-spill-word":
                np.bitwise_or.at(bits, (b0 >> 5) + j + 1, np.where(sh > 0, w >> back, 0).astype(np.uint32))
            prev = w
        before = prev
        if fault != "no-chunk-carry":
            carry = carry ^ below
    return bits[:field]
