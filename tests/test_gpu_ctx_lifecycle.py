"""What Context.close() (dsort_finalize) gives back.  A context owns some 45 grow-only arenas, pinned
host buffers, events and streams; one that close() forgot would leak on every open / close cycle.
Free device memory (torch.cuda.mem_get_info: the whole device's, so the inputs are allocated once,
before the first cycle, and every cycle reuses them) is sampled after the first and after the last of
eight cycles; the two must differ by less than what ONE cycle's context holds, measured in the first
cycle as free-after-close minus free-before-close."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CYCLES = 8
N = 1 << 23


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def run_cycles(dsort_mod, work):
    """`work(ctx)` in CYCLES fresh contexts.  Returns (the first cycle's footprint, free memory after
    the first close, free memory after the last)."""
    footprint = after_first = None
    for c in range(CYCLES):
        ctx = dsort_mod.Context(0)
        try:
            work(ctx)
            ctx.synchronize()
            held = free_bytes()
        finally:
            ctx.close()
        after = free_bytes()
        if c == 0:
            footprint, after_first = after - held, after
    return footprint, after_first, after


def test_open_use_close_cycles_do_not_leak(dsort_mod):
    k32 = torch.randint(-2 ** 31, 2 ** 31 - 1, (N,), dtype=torch.int32, device="cuda")
    k64 = torch.randint(-2 ** 62, 2 ** 62, (N,), dtype=torch.int64, device="cuda")
    vals = torch.arange(N, dtype=torch.int32, device="cuda")
    rows = torch.arange(2 * N, dtype=torch.int64, device="cuda").view(N, 2)  # 16-byte records
    o32, o32b, o64, orows = torch.empty_like(k32), torch.empty_like(k32), torch.empty_like(k64), torch.empty_like(rows)
    tk, ti = torch.empty(1024, dtype=torch.int32, device="cuda"), torch.empty(1024, dtype=torch.int32, device="cuda")
    text = torch.empty(12 * N, dtype=torch.uint8, device="cuda")

    def work(ctx):
        ctx.sort_dev(k32, out=o32)
        ctx.sort_pairs_dev(k32, vals, keys_out=o32, vals_out=o32b)
        with ctx.options(argsort_wide=1):
            ctx.argsort_dev(k64, idx_out=o32b, keys_out=o64)
        ctx.sort_records_dev(k64, rows, keys_out=o64, out=orows)
        with ctx.options(topk_path=1):
            ctx.topk_dev(k32, 1024, keys_out=tk, idx_out=ti)
        nbytes = ctx.format_text(k32, text)
        assert ctx.parse_text(text, nbytes, o32) == N

    work_once = dsort_mod.Context(0)  # (torch's and the runtime's own first-use allocations, outside the samples)
    work(work_once)
    work_once.close()
    footprint, first, last = run_cycles(dsort_mod, work)
    print(f"footprint of one cycle {footprint / 2 ** 20:.1f} MiB, free after cycle 1 {first / 2 ** 20:.1f} MiB, "
          f"after cycle {CYCLES} {last / 2 ** 20:.1f} MiB")
    assert footprint >= 16 * N  # (at least the pair arena and the wide path's second arena: 8 bytes a key each)
    assert abs(first - last) < footprint, (footprint, first, last)


def test_cycles_with_a_communicator_do_not_leak(dsort_mod):
    """The same with a one-rank communicator created and destroyed inside every cycle, around the
    sample sort and the distributed gather: dsort_comm_destroy followed by close leaves nothing."""
    n = 100_003
    k32 = torch.randint(-1000, 1000, (n,), dtype=torch.int32, device="cuda")
    k64 = torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64, device="cuda")
    rows = torch.arange(4 * n, dtype=torch.int32, device="cuda").view(n, 4)
    idx = torch.randperm(n, device="cuda").to(torch.int32)
    out = torch.empty_like(rows)

    def work(ctx):
        ctx.comm_init(1, 0, dsort_mod.Context.unique_id())
        try:
            _, nout = ctx.sample_sort_dev(k32.clone())
            assert nout == n
            ctx.sample_argsort_dev(k64, 0)
            ctx.sample_gather_dev(rows, 0, idx, out=out)
        finally:
            ctx.comm_destroy()

    work_once = dsort_mod.Context(0)
    work(work_once)
    work_once.close()
    footprint, first, last = run_cycles(dsort_mod, work)
    print(f"footprint of one cycle {footprint / 2 ** 20:.1f} MiB, free after cycle 1 {first / 2 ** 20:.1f} MiB, "
          f"after cycle {CYCLES} {last / 2 ** 20:.1f} MiB")
    assert footprint > 0
    assert abs(first - last) < footprint, (footprint, first, last)


def test_second_close_is_a_no_op(dsort_mod):
    """Context.close() drops its handle, so dsort_finalize never sees a context twice."""
    ctx = dsort_mod.Context(0)
    ctx.sort_dev(torch.randint(0, 100, (1000,), dtype=torch.int32, device="cuda"))
    ctx.synchronize()
    ctx.close()
    assert ctx.h is None
    ctx.close()
    assert ctx.h is None
