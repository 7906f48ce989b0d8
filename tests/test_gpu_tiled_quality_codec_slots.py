"""`codec.TiledQualityCodec` steps on poisoned slots between guard bands: tests/test_gpu_quality_codec_slots.py's procedure. Every
device buffer of the codec's slots lies between guard bands, the bands are verified after every step, and every SCRATCH buffer of
`_Slot` (tests/slot_buffers.py) and of `_TiledQualitySlot` (tests/tiled_quality_slot_buffers.py) is filled with the poison between two
steps -- the bisection's state, trace and accumulator, the thresholds, the probes' latent buffer and the coder's rows per stream among
them: a step that read what the step before it left would land elsewhere, and a round that wrote its rows outside `prob_row` would
break a band. The tickets are held against tests/test_gpu_tiled_quality_codec.py's reference, exactly."""
import pytest
import torch

import guarded
import slot_buffers
import tiled_quality_slot_buffers
from test_gpu_quality_codec import BATCH, assert_reference_coverage, check_step, thresholds_of_step
from test_gpu_tiled_quality_codec import build, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def references(tmp_path_factory):
    return {'directory': tmp_path_factory.mktemp('tiled_quality_slots')}


@pytest.mark.parametrize('poison', [0xFF, 0x7F], ids=['poison_ff', 'poison_7f'])
@pytest.mark.parametrize('mode', ['graphs', 'launches'])
def test_steps_on_poisoned_slots_between_guard_bands(references, mode, poison):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    ref = reference(references, 'fixed_L10_exception', (4, 4))
    images = torch.from_numpy(ref['images']).cuda()
    assert_reference_coverage(ref, 9)
    table = tiled_quality_slot_buffers.TILED_QUALITY_SLOT

    def between_steps(c, guard):
        c.drain()
        guard.check(keep=True)
        assert slot_buffers.poison_scratch(c, poison) > 0 and tiled_quality_slot_buffers.poison_scratch(c, poison) > 0

    with guarded.guarded((device, pipeline, codec), poison) as guard:
        with build(ref, mode) as c:
            for owner in tiled_quality_slot_buffers.quality_slots(c):
                assert slot_buffers.check_tiling(owner, table) == ['accum', 'select', 'table']
                scratch = {name for (name, _) in slot_buffers.scratch_leaves(owner, table)}
                assert set(tiled_quality_slot_buffers.MUST_BE_SCRATCH) <= scratch
                assert tuple(owner.hist.shape) == (BATCH, 3, 12, 128, 11) and owner.prob_row.numel() == BATCH*12*128
                assert sum(rows.numel() for rows in owner.class_rows) == owner.prob_row.numel()
            for (owner, slot_table) in slot_buffers.owners(c):
                assert 'block' in slot_buffers.check_tiling(owner, slot_table)
            torch.cuda.synchronize()
            between_steps(c, guard)
            for step in range(2*c.nb_slots + 1):
                thresholds = thresholds_of_step(ref, step)
                check_step(ref, c.submit(images, max_sse=thresholds), thresholds, step)
                between_steps(c, guard)
