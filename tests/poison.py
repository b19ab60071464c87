"""Test-side check that a HIP path never depends on what freed device memory last held (test infrastructure, never imported by the product).

The host code takes most of its buffers from `torch.empty`; the kernels are trusted to write every halo row, padded channel and slab
entry that something reads later.  In a test process the caching allocator hands a path either fresh (zero) memory or the block the same
tensor occupied one pass earlier, so a read of an unwritten entry sees a correct value.  This module takes that luck away:

`poison_free_memory(byte)` fills every block the allocator holds but has not handed out with one repeated byte; `run_on_patterns(fn)` runs
`fn` once per byte and returns the results, and `assert_same_bits` compares them.  The bytes and what they become:

    byte   fp32               bf16               fp64       int32        uint8 mask
    0x00   0                  0                  0          0            false
    0xFF   NaN                NaN                NaN        -1           true
    0x7F   3.396e38 (finite)  3.39e38 (finite)   1.38e306   2139062143   true

NaN spreads through sums and products but max(x, 0), fmaxf and comparisons swallow it; the huge finite value survives those.  Zero is
what fresh memory usually holds: the baseline that hides everything.

Two conditions are asserted here, not left to the caller: the poison reaches `torch.empty` (a block freed before the poisoning reads back
as the byte), and a poisoned run is served from poisoned memory alone (the allocator's reserved bytes do not grow during it).
"""
import torch

PATTERNS = (0x00, 0x7F, 0xFF)          # the all-ones pattern last: a case is first seen with the two patterns that stay finite
_SMALL = 1 << 20          # the allocator's small pool serves requests up to 1 MiB; a larger request never lands in a small segment
LAST = {}                 # figures of the latest poison_free_memory / run_on_patterns call (printed by the tests that quote them)


def _inactive(dev):
    """[(stream, pool, bytes)] of every block of device `dev` that the caching allocator holds and has not handed out"""
    out = []
    for seg in torch.cuda.memory_snapshot():
        # a captured graph keeps a private pool (segment_pool_id != (0, 0)): the allocator hands its blocks to nothing but that graph's
        # capture, so they can neither be poisoned from outside nor reach a torch.empty of an eager run
        if seg['device'] != dev or tuple(seg.get('segment_pool_id', (0, 0))) != (0, 0):
            continue
        for b in seg['blocks']:
            if b['state'] == 'inactive' and b['size'] >= 512:
                out.append((seg['stream'], seg['segment_type'], b['size']))
    return out


def _stream_of(raw, dev):
    # a segment belongs to the stream it was first allocated on; only that stream's requests are served from it
    return torch.cuda.default_stream(dev) if raw == 0 else torch.cuda.ExternalStream(raw, device=dev)


def poison_free_memory(byte, device=None):
    """Fill every free block of the caching allocator with `byte`, then free them again.  Returns (blocks, bytes) poisoned."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    torch.cuda.synchronize(dev)
    reserved = torch.cuda.memory_stats(dev)['reserved_bytes.all.current']
    held, nblocks, nbytes = [], 0, 0
    for _ in range(64):
        free = sorted(_inactive(dev), key=lambda e: -e[2])          # largest first, so nothing is split
        if not free:
            break
        for raw, pool, size in free:
            # a whole free small segment is 2 MiB, more than the small pool's largest request: take it in pieces (the next round takes the rest)
            take = min(size, _SMALL) if pool == 'small' else size
            with torch.cuda.stream(_stream_of(raw, dev)):
                t = torch.empty(take, dtype=torch.uint8, device='cuda:%d' % dev)
                t.fill_(byte)
            held.append(t)
            nblocks, nbytes = nblocks + 1, nbytes + take
    else:
        raise AssertionError('poison_free_memory: free blocks remain after 64 rounds: %r' % (_inactive(dev)[:8],))
    torch.cuda.synchronize(dev)
    assert not _inactive(dev), 'poison_free_memory: a free block was left unfilled'
    grown = torch.cuda.memory_stats(dev)['reserved_bytes.all.current'] - reserved
    # a request that fits no free block makes the allocator reserve a new segment; that one is filled like the others above, so growth here
    # costs nothing in coverage - it is recorded, and what matters (no growth during the run that follows) is asserted by run_on_patterns
    del held, t
    torch.cuda.synchronize(dev)
    LAST.update(byte=byte, blocks=nblocks, bytes=nbytes, reserved=reserved + grown, grown_while_poisoning=grown)
    return nblocks, nbytes


def _probe(byte, sizes, dev):
    """condition 1: right after the poisoning, torch.empty of sizes that were free before it reads back as all `byte`"""
    for raw, _, size in sizes:
        with torch.cuda.stream(_stream_of(raw, dev)):
            t = torch.empty(size, dtype=torch.uint8, device='cuda:%d' % dev)
            ok = bool((t.cpu() == byte).all())          # compared on the host: a device-side compare would allocate, and leave, an unpoisoned block
        assert ok, 'poison 0x%02X did not reach torch.empty(%d)' % (byte, size)
        del t


def to_cpu(r):
    if isinstance(r, torch.Tensor):
        return r.detach().cpu().clone()
    if isinstance(r, dict):
        return {k: to_cpu(v) for k, v in r.items()}
    if isinstance(r, (list, tuple)):
        return [to_cpu(v) for v in r]
    return r


def run_on_patterns(fn, patterns=PATTERNS, device=None):
    """fn() once to warm the allocator (result dropped), then once per pattern on poisoned memory; the results, cloned to the CPU.
    A stateful case (a training run) takes one argument, `fn(repoison)`, and calls `repoison()` between its steps: nothing in the warm run,
    a fresh poisoning with the pattern at hand in the others."""
    import inspect
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    stats = lambda: torch.cuda.memory_stats(dev)['reserved_bytes.all.current']      # noqa: E731
    stateful = len(inspect.signature(fn).parameters) == 1
    to_cpu(fn(lambda: None) if stateful else fn())
    results, figures = [], []
    for byte in patterns:
        for attempt in range(2):
            torch.cuda.synchronize(dev)
            before_free = _inactive(dev)
            assert before_free, 'nothing was freed by the warm run: the case allocates no device memory'
            nblocks, nbytes = poison_free_memory(byte, dev)
            # the probe: the smallest and the largest block (<= 64 MiB, to keep the read cheap) that were free before the poisoning
            cand = sorted((e for e in before_free if e[2] <= (_SMALL if e[1] == 'small' else 64 << 20)), key=lambda e: e[2])
            _probe(byte, [cand[0], cand[-1]] if cand else [], dev)
            torch.cuda.synchronize(dev)
            before = stats()
            again = [0]

            def repoison():
                poison_free_memory(byte, dev)
                again[0] += LAST['grown_while_poisoning']        # a segment reserved BY the poisoning is poisoned memory: not the run's growth

            r = to_cpu(fn(repoison) if stateful else fn())
            torch.cuda.synchronize(dev)
            after = stats() - again[0]
            if after == before:
                break
            # part of this run was served from memory reserved during it (fresh, not poisoned): it was one more warm run; once more
            del r
        assert after == before, ('pattern 0x%02X: reserved bytes grew %d -> %d during the poisoned run, also after a second warm run: '
                                 'part of it ran on fresh memory' % (byte, before, after))
        results.append(r)
        figures.append(dict(byte=byte, blocks=nblocks, bytes=nbytes, reserved_before=before, reserved_after=after, attempts=attempt + 1))
    LAST['runs'] = figures
    return results


def _flat(r, path='r'):
    if isinstance(r, torch.Tensor):
        yield path, r
    elif isinstance(r, dict):
        for k in r:
            yield from _flat(r[k], '%s[%r]' % (path, k))
    elif isinstance(r, (list, tuple)):
        for i, v in enumerate(r):
            yield from _flat(v, '%s[%d]' % (path, i))
    elif r is not None:
        yield path, torch.as_tensor(r)


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same_bits(a, b):
    """torch.equal on an integer view of the same width, so that NaNs compare equal to themselves"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.bool or a.numel() == 0:
        return torch.equal(a, b)
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    it = _INT[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def differences(results, patterns=PATTERNS):
    """['r[2] differs between 0x00 and 0xFF: ...'] for every tensor of a later result that is not the first result's bits"""
    out = []
    base = list(_flat(results[0]))
    for byte, other in zip(patterns[1:], results[1:]):
        cur = list(_flat(other))
        if [p for p, _ in cur] != [p for p, _ in base]:
            out.append('the result has another structure on pattern 0x%02X' % byte)
            continue
        for (p, u), (_, v) in zip(base, cur):
            if not same_bits(u, v):
                if u.shape == v.shape and u.dtype == v.dtype:
                    uf, vf = (torch.view_as_real(u), torch.view_as_real(v)) if u.is_complex() else (u, v)
                    bad = ~((uf == vf) | (torch.isnan(uf.double()) & torch.isnan(vf.double())))
                    where = 'at %d of %d entries, first %r' % (int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()) if bad.any() else ())
                else:
                    where = 'shape / dtype %r %r against %r %r' % (tuple(u.shape), u.dtype, tuple(v.shape), v.dtype)
                out.append('%s differs between patterns 0x%02X and 0x%02X %s' % (p, patterns[0], byte, where))
    return out


def not_finite(results, patterns=PATTERNS):
    out = []
    for byte, r in zip(patterns, results):
        for p, t in _flat(r):
            if (t.is_floating_point() or t.is_complex()) and not bool(torch.isfinite(t).all()):
                out.append('%s is not finite on pattern 0x%02X (%d entries)' % (p, byte, int((~torch.isfinite(t)).sum())))
    return out


def assert_same_bits(fn, patterns=PATTERNS, device=None):
    """the assertion of a path that adds in fixed orders: identical inputs, so any difference between the patterns is a read of memory the
    path did not write.  Returns the first result."""
    results = run_on_patterns(fn, patterns, device)
    n = sum(1 for _ in _flat(results[0]))
    assert n > 0, 'the case returns no tensor'
    bad = not_finite(results, patterns) + differences(results, patterns)
    assert not bad, 'the path reads memory it did not write:\n  ' + '\n  '.join(bad[:20])
    return results[0]
