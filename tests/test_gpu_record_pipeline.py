"""The queue kernel's record pipeline, against the oracle.

On open a group's ciphertext is GHASHed inside that group's own AES rounds
(gcm_device.h gcm_blocks_xN): the first group of a record runs the hook like
every other (in the no-pack kernels at later rounds than the groups after
it), no GHASH step trails the loop, and a record of one group has first group
= last group.  A wave takes record after record from its run's queue, so the
batches here are shaped by how many records a wave takes in a session run
and by what kind of record sits on either side of a good one.  They complement
test_gpu_record_handover (whose plans they follow): runs that lie whole inside
a workgroup's range, special records as a run's first record and as the
batch's last, and the group boundaries of the wide loop as lengths.  Every
output byte, tag and status is compared with the oracle's
tls1_enc; output and status start from a sentinel and each batch runs twice on
fresh buffers (the helpers of test_gpu_record_handover).

Every batch holds more than 4096 records, so a workgroup's range is longer
than its 16 waves and waves take a second and a third record.  Records are
short, the workload's own 16 KiB aside.
"""
import pytest

from test_gpu_record_handover import (EMPTY, INVALID, KINDS, NSESS, OOB, TAMPER,  # noqa: F401
                                      VARIANTS, _run_case, engine, queue_impl, ta)

pytestmark = pytest.mark.gpu

# no group (0, 1: the tail loops alone), one group of two steps (first group =
# last group), one group and an odd step, two groups, and 128 groups
LENS = [0, 1, 2048, 2064, 3072, 4096, 16384]
SHORT = LENS[:-1]
RUN_SHAPES = (1, 2, 15, 16, 17, 33)   # 84 records: one workgroup's range, see _shapes_plan


def _shapes_plan(cus):
    """One cycle of the run shapes per CU, in turn forwards and backwards.  The
    engine gives each of its workgroups (one per CU) ceil(n / CUs) records:
    84 when `cus` is the GPU's own CU count (21504 records on 256 CUs), so
    every range then holds whole runs of 1 (every claim past the first
    returns >= run_end), 2, 15 (no wave takes a second record), 16, 17 (one
    wave takes a second) and 33 (waves take a second and a third).  On a GPU
    with fewer than 49 CUs the caller passes 49 to keep the batch above 4096
    records; the ranges then cut runs where they fall, which the comparison
    with the oracle covers as well, but the whole-run property holds only
    from 49 CUs on.  With an even `cus` the last cycle runs backwards: the
    batch ends with a run of one record, run_end = the batch's record count.
    Sessions change with every run; the short lengths in turn and every 29th
    record 16 KiB."""
    plan, k, run = [], 0, 0
    for c in range(cus):
        for run_len in (RUN_SHAPES if c % 2 == 0 else RUN_SHAPES[::-1]):
            for _ in range(run_len):
                plan.append((run % NSESS, 16384 if k % 29 == 28 else SHORT[k % len(SHORT)]))
                k += 1
            run += 1
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_run_shapes(ta, engine, oracle, queue_impl, name, mode, hints):
    """Runs of 1, 2, 15, 16, 17 and 33 records inside one workgroup's range: no
    record taken twice or left out (its status would keep the sentinel), none
    claimed across a run's end, the last run ending at the batch's last record."""
    cus = max(engine.num_cus, 49)
    _run_case(ta, engine, oracle, name, mode, hints, "pipe-shapes-%d" % cus, _shapes_plan(cus))


def _neighbour_plan(mode, last):
    """256 runs of 24 records (6144 records): in every run a special record
    between two good ones (position 3: directly after one and directly before
    one), one as the run's last record, directly before the next run's first,
    and in every other run one as the run's first record, directly after the
    previous run's end; the kinds rotate over the runs.  The batch's last record
    is of kind `last`.  An empty-session record is a run of its own, so there
    the good records before it end a run one record early."""
    kinds = [OOB, EMPTY] + ([TAMPER, INVALID] if mode == "open" else [])
    plan, special = [], {}
    for run in range(256):
        for j in range(24):
            k = 24 * run + j
            plan.append((run % NSESS, 16384 if k % 31 == 30 else SHORT[(run + 5 * j) % len(SHORT)]))
        special[24 * run + 3] = kinds[run % len(kinds)]
        special[24 * run + 23] = kinds[(run // len(kinds) + 1) % len(kinds)]
        if run % 2:
            special[24 * run] = kinds[(run // 2) % len(kinds)]
    special[len(plan) - 1] = last
    return plan, special


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode,last", [("seal", OOB), ("seal", EMPTY), ("open", TAMPER),
                                       ("open", OOB), ("open", INVALID), ("open", EMPTY)])
@pytest.mark.parametrize("name", list(KINDS))
def test_neighbours(ta, engine, oracle, queue_impl, name, mode, last, hints):
    """A tampered record (zero-filled while its neighbours' loads and stores
    are in flight), an out-of-bounds descriptor, a publicly invalid length and
    an empty session directly before and after good records, as the last
    record of a run and as the last record of the batch: exact statuses,
    zeros for BAD_MAC only, nothing else written."""
    plan, special = _neighbour_plan(mode, last)
    _run_case(ta, engine, oracle, name, mode, hints, "pipe-neighbours", plan, special=special)


def _lengths_plan():
    """Every ordered pair of LENS as neighbours, one 98-record sequence per
    session run, rotated from run to run: 84 runs, 8232 records, 33 per
    workgroup, so ranges end inside runs and a wave's first, second and third
    record have every length."""
    seq = [n for a in LENS for b in LENS for n in (a, b)]
    plan = []
    for run in range(84):
        rot = (29 * run) % len(seq)
        plan += [(run % NSESS, n) for n in seq[rot:] + seq[:rot]]
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_lengths_and_alignment(ta, engine, oracle, queue_impl, name, mode, hints):
    """0, 1, 2048, 2064, 3072, 4096 and 16384 bytes next to each other, in one
    batch that mixes 16-byte-aligned slots (the wide step loop) with shifted
    ones (the tail loops for the whole record)."""
    plan = _lengths_plan()
    shifts = [0 if i % 3 != 2 else 1 + (i // 3) % 15 for i in range(len(plan))]
    _run_case(ta, engine, oracle, name, mode, hints, "pipe-lengths", plan, shifts=shifts)
