"""The host side of the reference's InSpatio-World infill step (inspatio_world_infill.py, iwi:) around the device's masked alignment
(include/mdvt_inspatio.h; the wrapper that hands tensors to it is inspatio_device.py's).  No torch and no tensor address here:
NumPy on what one read-back per chunk and eye brings -- the 4 x 4 shifts and their status bytes.

  pad_to_valid_T   the frame count the video model is handed (iwi:225-236)
  chunk_schedule   225 frames per chunk, 6 kept, as infill_clip's schedule with the chunk length as a parameter
  clean_grid       one frame's shifts to its flow grid: the 20-pixel limit, the MAD rule, the fill from neighbours (iwi:61-73, 110-127)
  flow_grids       a chunk's flow grids, each the mean with the previous frame's where that frame has one (iwi:170-181)

On the device as well (include/mdvt_inspatio.h): the frame preparation with the hole counts flow_grids takes, and the flow warp that
takes its grids, and the compositing with its edge blending.  The tool around a generator is tools/inspatio_world_infill.py.
movie_2_3D keeps refusing --infill_engine inspatio_world: wiring the engine into the driver is a follow-up (README).

DECREES ("InSpatio-World alignment").  The MAD rule runs on float32 values with float32 results, as NumPy 2 evaluates
iwi:121-124: median and mad are float32, mad = fl32(fl32(median(|v - median|)) + fl32(1e-8)).  A mean of k grids or neighbours is
the float32 sum in their order divided by float32(k).
"""
from __future__ import annotations

import numpy as np

FRAMES_CHUNK, OVERLAP = 225, 6            # iwi:42; the six kept frames are infill_clip's
GRID = 4                                  # iwi:55-56
MAX_SHIFT = 20                            # iwi:110
F = np.float32


def latent_frames(T: int) -> int:
    """Latent frames the video model's VAE makes of T frames (iwi:220-222)."""
    return (T + 3) // 4


def pad_to_valid_T(T: int, frames_per_block: int = 3) -> int:
    """The smallest T' >= T of the form 4 k - 3 whose k latent frames are a multiple of frames_per_block (iwi:225-236)."""
    if T < 1:
        raise ValueError("a chunk needs at least one frame")
    k = -(-latent_frames(T) // frames_per_block) * frames_per_block
    while 4 * k - 3 < T:
        k += frames_per_block
    return 4 * k - 3


def chunk_schedule(n_frames: int, chunk: int = FRAMES_CHUNK):
    """The calls of the chunk schedule for a clip of n_frames: [(first, last, frame of the buffer's index 0, buffered frames, (a, b))],
    where [a, b) are the clip's frames the call writes.  After a call the buffer keeps six frames: three pasted ones with their own
    masks, then three untouched ones; a call writes from its index 3 unless it is the first and stops 3 short unless it is the last."""
    if n_frames < 1:
        raise ValueError("a clip needs at least one frame")
    if chunk <= OVERLAP:
        raise ValueError(f"a chunk must be longer than the {OVERLAP} frames kept between chunks")
    calls, first, base, held = [], True, 0, 0
    for _ in range(n_frames):
        held += 1
        if held >= chunk:
            calls.append((first, False, base, held, (base + (0 if first else 3), base + held - 3)))
            first, base, held = False, base + held - OVERLAP, OVERLAP
    calls.append((first, True, base, held, (base + (0 if first else 3), base + held)))
    return calls


def _mean32(values):
    """The float32 sum of `values` (arrays of one shape) in their order, divided by float32(their number)."""
    total = np.array(values[0], F)
    for v in values[1:]:
        total = (total + np.asarray(v, F)).astype(F)
    return (total / F(len(values))).astype(F)


def clean_grid(shift, status):
    """shift float64 [4, 4, 2] (dy, dx) and status [4, 4] of one frame, as mdvt_masked_shift_grid writes them -> the frame's flow
    grid, float32 [4, 4, 2] (dx, dy).  A cell is reliable where it was computed, within 20 pixels on both axes and, where more than one
    cell is, no further than 2 mad from the median on either channel; the others take the mean of their reliable 8-neighbours, in
    row-major order, reading the grid as it is being updated (a cell without a reliable neighbour stays 0)."""
    shift, status = np.asarray(shift, np.float64), np.asarray(status)
    if shift.shape != (GRID, GRID, 2) or status.shape != (GRID, GRID):
        raise ValueError(f"shift must be (4, 4, 2) and status (4, 4), got {shift.shape} and {status.shape}")
    flow = np.zeros((GRID, GRID, 2), F)
    unreliable = np.ones((GRID, GRID), bool)
    for gy in range(GRID):
        for gx in range(GRID):
            dy, dx = float(shift[gy, gx, 0]), float(shift[gy, gx, 1])
            if not status[gy, gx] or abs(dx) > MAX_SHIFT or abs(dy) > MAX_SHIFT:
                continue
            flow[gy, gx] = (dx, dy)
            unreliable[gy, gx] = False
    computed = ~unreliable
    if computed.sum() > 1:
        for ch in range(2):
            vals = flow[computed, ch]
            median = F(np.median(vals))
            mad = F(F(np.median(np.abs(vals - median).astype(F))) + F(1e-8))
            unreliable |= computed & (np.abs(flow[..., ch] - median).astype(F) > F(2.0) * mad)
    for gy, gx in zip(*np.where(unreliable)):
        near = [flow[gy + dy, gx + dx].copy() for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if (dy or dx) and 0 <= gy + dy < GRID and 0 <= gx + dx < GRID and not unreliable[gy + dy, gx + dx]]
        if near:
            flow[gy, gx] = _mean32(near)
    return flow


def flow_grids(shifts, statuses, hole_counts):
    """A chunk's flow grids: shifts [T, 4, 4, 2], statuses [T, 4, 4], hole_counts [T] -> (grids float32 [T, 4, 4, 2], has_grid uint8
    [T]).  A frame without a hole has no grid (iwi:160-163); a frame's grid is the mean of the previous frame's cleaned grid, where
    that frame has one, and its own (iwi:175-181)."""
    T = len(hole_counts)
    grids, has = np.zeros((T, GRID, GRID, 2), F), np.zeros(T, np.uint8)
    cleaned = [clean_grid(shifts[i], statuses[i]) if int(hole_counts[i]) > 0 else None for i in range(T)]
    for i in range(T):
        if cleaned[i] is None:
            continue
        own = [g for g in (cleaned[i - 1] if i > 0 else None, cleaned[i]) if g is not None]
        grids[i], has[i] = _mean32(own), 1
    return grids, has
