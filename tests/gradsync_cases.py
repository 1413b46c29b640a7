"""The tensor set of the gradient-bucket tests (tests/test_gradsync_gpu.py, tests/test_redzone_gradsync_gpu.py): every length and alignment
at which csrc/gradsync.hip takes another path.

  * lengths 1, 3, 7 (below one quad, head and tail only), 64, 4099 (one chunk and three words), 82 944 (the largest weight: 21 chunks);
  * a view whose ``data_ptr() % 16 == 4`` (the source's phase differs from most slots');
  * 8 197 elements with source and slot both on a 16-byte boundary (whole chunks through the form without bounds tests);
  * fillers cut from one buffer back to back, so their sources sit at every phase, up to ``TABLE + 1`` entries: the second launch runs;
  * a ``None`` entry (zeros);
  * slots in list order with gaps of 1, 2, 3, 5 words between them, so slot offsets take every phase and mostly are no multiple of 4.

The 7-element tensor holds NaN, +Inf and -Inf.  Everything is a function of the seed, built on the CPU and moved by the caller.
"""
import torch

TABLE = 128                       # virnet_amd.dist.GRADSYNC_TABLE
LENGTHS = (1, 3, 7, 64, 4099, 82944)
VIEW_LEN = 263
ALIGNED_LEN = 2 * 4096 + 5
NULL_LEN = 5
SENTINEL = -7777.25
GAPS = (1, 2, 3, 5)
I_SPECIAL = 2                     # the 7-element tensor
I_VIEW = len(LENGTHS)
I_ALIGNED = I_VIEW + 1
I_NULL = I_ALIGNED + 1
COUNT = TABLE + 1


def make_tensors(device, wrap=lambda t: t, seed=0):
    """-> (tensors: COUNT entries, one of them None; sizes; the buffer the view lives in; the fillers' buffer).  ``wrap`` places a
    device tensor (the red-zone test moves it into an arena)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda n: (torch.rand(n, generator=gen) - 0.5) * 3.0
    tensors = [wrap(rnd(n).to(device)) for n in LENGTHS]
    tensors[I_SPECIAL][1:4] = torch.tensor([float("nan"), float("inf"), float("-inf")], device=device)
    view_buf = wrap(rnd(VIEW_LEN + 9).to(device))
    tensors.append(view_buf[1:1 + VIEW_LEN])
    tensors.append(wrap(rnd(ALIGNED_LEN).to(device)))
    tensors.append(None)
    fill_sizes = [1 + (7 * k) % 41 for k in range(COUNT - len(tensors))]
    fill_buf = wrap(rnd(sum(fill_sizes)).to(device))
    pos = 0
    for n in fill_sizes:
        tensors.append(fill_buf[pos:pos + n])
        pos += n
    sizes = [NULL_LEN if t is None else t.numel() for t in tensors]
    assert len(tensors) == COUNT and tensors[I_VIEW].data_ptr() % 16 == 4 and tensors[I_ALIGNED].data_ptr() % 16 == 0
    return tensors, sizes, view_buf, fill_buf


def make_offsets(sizes):
    """-> (offsets, bucket length).  The aligned tensor's slot starts on a multiple of 4, every other slot follows its predecessor after
    a gap; the bucket ends with a tail of 6 words that belong to no slot."""
    offsets, cur = [], 1
    for i, n in enumerate(sizes):
        if i == I_ALIGNED:
            cur = -(-cur // 4) * 4
        offsets.append(cur)
        cur += n + GAPS[i % len(GAPS)]
    assert sum(1 for o in offsets if o % 4) > len(offsets) // 2 and offsets[I_ALIGNED] % 4 == 0
    return offsets, cur + 6


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)
