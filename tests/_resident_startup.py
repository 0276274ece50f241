"""The start-up sum of k_pcg_resident (engine_pcg_resident.h), restated in numpy float64 for the tests.

k_pcg_init leaves one partial of ||b||^2 per workgroup (gridM of them, at most 1024).  Wavefront 0 of every workgroup of the resident
launch sums them: lane l adds the partials l, l + 64, l + 128, ... in ascending order, starting from 0.0; the 64 lane sums go through
wave_sum -- four butterfly steps inside rows of 16 lanes (partner lane ^ 1, lane ^ 2, the mirror inside 8 lanes, the mirror inside 16
lanes), then (row 0 + row 1) + (row 2 + row 3); tol2 = max((eps_rel * eps_rel) * bb, eps_abs * eps_abs)."""
import numpy as np

LANES = 64
MAX_PARTS = 1024


def lane_sums(part):
    """The 64 lane sums: each lane's partials in ascending order from 0.0, one float64 addition per partial."""
    part = np.asarray(part, np.float64)
    acc = np.zeros(LANES)
    for q in range(0, part.size, LANES):
        chunk = part[q:q + LANES]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    return acc


def wave_sum(v):
    """engine_device.h's wave_sum on 64 lane values, addition by addition."""
    v = np.asarray(v, np.float64).copy()
    i = np.arange(LANES)
    for partner in (i ^ 1, i ^ 2, (i & ~7) | (7 - (i & 7)), (i & ~15) | (15 - (i & 15))):
        v = v + v[partner]
    return (v[0] + v[16]) + (v[32] + v[48])


def start_sum(part):
    return wave_sum(lane_sums(part))


def tol2(part_bb, eps_rel, eps_abs):
    bb = start_sum(part_bb)
    return max((np.float64(eps_rel) * np.float64(eps_rel)) * bb, np.float64(eps_abs) * np.float64(eps_abs))
