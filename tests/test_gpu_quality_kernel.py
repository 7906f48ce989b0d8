"""eae_hip_quality_search (csrc/hip/quality.hip; device.quality_search) driven through all of its rounds on poisoned buffers between
guard bands under both poisons (tests/guarded.py), against the host rule it restates in integers, ratecontrol.select_by_quality.

The test stands in for the synthesis pass: in front of round r >= 1 it writes into `probe_acc` the table's squared error of the point
the device left in `point`. After EVERY round it compares `point`, `prob_row`, `flags`, `state` and the whole trace with what the rule
gives at that round, and asks `probe_acc` to be zero; after the last round the choice is select_by_quality's. N = 1, 3, 65, K = 1..9,
with and without an exception map; tables monotone and arbitrary, squared errors beyond 32 bits, thresholds at an entry, one under it
and under all of them. Every comparison is exact."""
import numpy
import pytest

pytestmark = pytest.mark.gpu

NB_MAPS = 128


@pytest.fixture(autouse=True, params=[0xFF, 0x7F], ids=['poison_ff', 'poison_7f'])
def guard(request):
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), request.param) as g:
        yield g


@pytest.fixture(scope='module')
def dev():
    from autoencoder_based_image_compression_amd import device
    return device


@pytest.fixture(scope='module')
def rc():
    from autoencoder_based_image_compression_amd import ratecontrol
    return ratecontrol


def case(n, k_points, seed):
    """(sse int64 (n, K), first int64 (n,), max_sse int64 (n,)): even images monotone, odd ones arbitrary, every third beyond 2^40."""
    rng = numpy.random.RandomState(seed)
    sse = numpy.zeros((n, k_points), dtype=numpy.int64)
    for i in range(n):
        row = 1000 + numpy.cumsum(rng.randint(0, 500, size=k_points)) if i % 2 == 0 else rng.randint(0, 5000, size=k_points)
        sse[i] = row.astype(numpy.int64) + ((1 << 40) if i % 3 == 2 else 0)
    first = rng.randint(0, k_points, size=n).astype(numpy.int64)
    max_sse = numpy.zeros(n, dtype=numpy.int64)
    for i in range(n):
        j = rng.randint(0, k_points + 1)
        max_sse[i] = sse[i, j] - rng.randint(0, 2) if j < k_points else sse[i].min() - 1
    return sse, first, max_sse


def states_by_round(sse, first, max_sse, nb_rounds):
    """(L, R) of every image behind round 0, 1, .., nb_rounds: int32 (nb_rounds + 1, n, 2), stepped as the issue states it."""
    (n, k_points) = sse.shape
    states = numpy.zeros((nb_rounds + 1, n, 2), dtype=numpy.int32)
    for i in range(n):
        (low, high) = (int(first[i]) - 1, k_points)
        states[0, i] = (low, high)
        for r in range(1, nb_rounds + 1):
            if high - low > 1:
                mid = (low + high) >> 1
                if sse[i, mid] <= max_sse[i]:
                    low = mid
                else:
                    high = mid
            states[r, i] = (low, high)
    return states


def rows_of(point, exception, row_base):
    prob_row = point.astype(numpy.int64)[:, None]*NB_MAPS + numpy.arange(NB_MAPS)[None, :]
    if exception >= 0:
        prob_row[:, exception] = row_base + numpy.arange(point.shape[0])
    return prob_row.astype(numpy.int32)


@pytest.mark.parametrize('exception', [-1, 5], ids=['no_exception', 'exception'])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_every_round_against_the_host_rule(dev, rc, guard, n, exception):
    import torch
    (met_seen, live_last_round) = (set(), 0)
    for k_points in range(1, 10):
        nb_rounds = rc.quality_rounds(k_points)
        row_base = k_points*NB_MAPS
        (sse, first, max_sse) = case(n, k_points, 1000*n + 10*k_points + (exception >= 0))
        (point_ref, met_ref, probe_points, probe_sse) = rc.select_by_quality(sse, first, max_sse)
        states = states_by_round(sse, first, max_sse, nb_rounds)
        buffers = {'first': guard.upload(first.astype(numpy.int32)), 'max_sse': guard.upload(max_sse),
                   'state': guard.empty((n, 2), dtype=torch.int32, device='cuda'), 'probe_acc': guard.empty(n, dtype=torch.int64, device='cuda'),
                   'point': guard.empty(n, dtype=torch.int32, device='cuda'), 'prob_row': guard.empty((n, NB_MAPS), dtype=torch.int32, device='cuda'),
                   'trace_point': guard.empty((n, nb_rounds), dtype=torch.int32, device='cuda'),
                   'trace_sse': guard.empty((n, nb_rounds), dtype=torch.int64, device='cuda'), 'flags': guard.empty(n, dtype=torch.int32, device='cuda')}
        table = torch.from_numpy(sse).cuda()
        for round in range(nb_rounds + 1):
            if round:
                # the synthesis pass: the squared error of the point the device asked for, added into the zeroed accumulator
                buffers['probe_acc'] += table.gather(1, buffers['point'].to(torch.int64)[:, None])[:, 0]
            dev.quality_search(*(buffers[name] for name in ('first', 'max_sse', 'state', 'probe_acc', 'point', 'prob_row', 'trace_point',
                                                            'trace_sse', 'flags')), k_points, round, exception, row_base)
            got = {name: t.cpu().numpy() for (name, t) in buffers.items()}
            last = round == nb_rounds
            point = point_ref if last else probe_points[:, round]
            where = (n, k_points, round)
            assert numpy.array_equal(got['point'], point.astype(numpy.int32)), where
            assert numpy.array_equal(got['prob_row'], rows_of(point, exception, row_base)), where
            assert numpy.array_equal(got['flags'], met_ref.astype(numpy.int32) if last else numpy.zeros(n, dtype=numpy.int32)), where
            assert numpy.array_equal(got['state'], states[round]), where
            trace_point = numpy.full((n, nb_rounds), -1, dtype=numpy.int32)
            trace_sse = numpy.full((n, nb_rounds), -1, dtype=numpy.int64)
            (trace_point[:, :round], trace_sse[:, :round]) = (probe_points[:, :round], probe_sse[:, :round])
            assert numpy.array_equal(got['trace_point'], trace_point) and numpy.array_equal(got['trace_sse'], trace_sse), where
            assert not got['probe_acc'].any(), where
            assert numpy.array_equal(got['first'], first.astype(numpy.int32)) and numpy.array_equal(got['max_sse'], max_sse), where
            guard.check(keep=True)
        met_seen.update(met_ref.tolist())
        live_last_round += int((states[nb_rounds - 1, :, 1] - states[nb_rounds - 1, :, 0] > 1).sum())
        guard.check()
    # over the nine ladders: images that met the threshold and images that did not, and a last round that still had to decide
    assert met_seen == {True, False} and live_last_round > 0


def test_every_round_writes_what_it_says(dev, rc, guard):
    """Outputs that held another fill come back the same from a whole search: nothing depends on what the buffers held."""
    import torch
    (n, k_points, exception) = (3, 9, 5)
    nb_rounds = rc.quality_rounds(k_points)
    (sse, first, max_sse) = case(n, k_points, 77)
    table = torch.from_numpy(sse).cuda()
    results = []
    for fill in (0x55, 0xAA):
        outs = {'state': torch.empty((n, 2), dtype=torch.int32, device='cuda'), 'probe_acc': torch.empty(n, dtype=torch.int64, device='cuda'),
                'point': torch.empty(n, dtype=torch.int32, device='cuda'), 'prob_row': torch.empty((n, NB_MAPS), dtype=torch.int32, device='cuda'),
                'trace_point': torch.empty((n, nb_rounds), dtype=torch.int32, device='cuda'),
                'trace_sse': torch.empty((n, nb_rounds), dtype=torch.int64, device='cuda'), 'flags': torch.empty(n, dtype=torch.int32, device='cuda')}
        for t in outs.values():
            t.view(torch.uint8).fill_(fill)
        (first_d, max_d) = (guard.upload(first.astype(numpy.int32)), guard.upload(max_sse))
        for round in range(nb_rounds + 1):
            if round:
                outs['probe_acc'] += table.gather(1, outs['point'].to(torch.int64)[:, None])[:, 0]
            dev.quality_search(first_d, max_d, outs['state'], outs['probe_acc'], outs['point'], outs['prob_row'], outs['trace_point'],
                               outs['trace_sse'], outs['flags'], k_points, round, exception, k_points*NB_MAPS)
        results.append({name: t.cpu().numpy() for (name, t) in outs.items()})
    for name in results[0]:
        assert numpy.array_equal(results[0][name], results[1][name]), name
    (point, met, _, _) = rc.select_by_quality(sse, first, max_sse)
    assert numpy.array_equal(results[0]['point'], point) and numpy.array_equal(results[0]['flags'], met.astype(numpy.int32))


def test_quality_search_refuses_bad_arguments(dev, rc, guard):
    import torch
    from autoencoder_based_image_compression_amd import _native
    lib = _native.hip()
    (n, k_points) = (3, 9)
    nb_rounds = rc.quality_rounds(k_points)
    inputs = (guard.upload(numpy.zeros(n, dtype=numpy.int32)), guard.upload(numpy.full(n, 10**6, dtype=numpy.int64)))
    outs = (torch.full((n, 2), -7, dtype=torch.int32, device='cuda'), torch.full((n + 1,), -7, dtype=torch.int64, device='cuda'),
            torch.full((n,), -7, dtype=torch.int32, device='cuda'), torch.full((n, NB_MAPS), -7, dtype=torch.int32, device='cuda'),
            torch.full((n, nb_rounds), -7, dtype=torch.int32, device='cuda'), torch.full((n + 1, nb_rounds), -7, dtype=torch.int64, device='cuda'),
            torch.full((n,), -7, dtype=torch.int32, device='cuda'))
    pointers = [t.data_ptr() for t in inputs + outs]
    call = lib.eae_hip_quality_search
    # (first, max_sse, state, probe_acc, point, prob_row, trace_point, trace_sse, flags, k_points, nb_rounds, round, exception, row base, n, stream)
    good = pointers + [k_points, nb_rounds, 0, 5, k_points*NB_MAPS, n, None]
    for position in range(9):                                     # a NULL pointer
        assert call(*(good[:position] + [None] + good[position + 1:])) == -1, position
    for (position, value) in ((9, 0), (9, -1), (10, nb_rounds - 1), (10, nb_rounds + 1), (11, nb_rounds + 1), (11, -1), (12, 128), (13, -1),
                              (14, 0), (14, -2), (1, pointers[1] + 4), (3, pointers[3] + 4), (7, pointers[7] + 4)):
        assert call(*(good[:position] + [value] + good[position + 1:])) == -1, (position, value)
    for k in range(1, 65):                                        # nb_rounds must be ceil(log2(k_points + 1)), whatever the round
        for rounds in range(0, 9):
            if rounds != rc.quality_rounds(k):
                assert call(*(good[:9] + [k, rounds, 0] + good[12:])) == -1, (k, rounds)
    assert call(*(good[:14] + [65536] + good[15:])) == -2         # EAE_HIP_BAD_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == -7).all().item()) for t in outs)        # nothing was launched
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert outs[2].cpu().tolist() == [4]*n and not bool((outs[1][:n] != 0).any().item())
    with pytest.raises(dev.HipError):
        dev.quality_search(inputs[0], inputs[1], outs[0], outs[1][:n], outs[2], outs[3], outs[4][:, :2].contiguous(), outs[5][:n], outs[6],
                           k_points, 0, 5, k_points*NB_MAPS)
    with pytest.raises(dev.HipError):
        dev.quality_search(inputs[0], inputs[1].to(torch.int32), outs[0], outs[1][:n], outs[2], outs[3], outs[4], outs[5][:n], outs[6],
                           k_points, 0, 5, k_points*NB_MAPS)
