"""`codec.BatchCodec(..., rdo_lambda=...)` steps on poisoned slots between guard bands: tests/test_gpu_codec_slots.py's procedure. Every
device buffer of the codec's slots lies between guard bands, the bands are verified after every step, and every SCRATCH buffer of
`_Slot` (tests/slot_buffers.py) is filled with the poison between two steps. The quantiser's thresholds and its `point` tensor are
constants of the codec, made in the constructor: the slot gains no buffer, so the inventory of tests/slot_buffers.py is complete as it
is (`check_tiling` walks every slot). The tickets are held against tests/test_gpu_rdo_codec.py's reference, exactly, and the values
under the two poisons are the same."""
import pytest
import torch

import guarded
import slot_buffers
from test_gpu_rdo_codec import build, check_step, reference

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F)


@pytest.fixture(scope='module')
def references():
    return {}


@pytest.mark.parametrize('name, mode', [('fixed_exception', 'graphs'), ('fixed_exception', 'launches'), ('fixed_tiles_4x4', 'graphs'),
                                        ('learned_exception', 'launches')])
def test_steps_on_poisoned_slots_between_guard_bands(references, name, mode):
    from autoencoder_based_image_compression_amd import codec, device, pipeline
    ref = reference(references, name)
    images = torch.from_numpy(ref['images']).cuda()
    seen = {}

    def between_steps(c, guard, poison):
        c.drain()
        guard.check(keep=True)
        assert slot_buffers.poison_scratch(c, poison) > 0

    for poison in POISONS:
        with guarded.guarded((device, pipeline, codec), poison) as guard:
            with build(ref, mode) as c:
                for (owner, table) in slot_buffers.owners(c):
                    assert 'block' in slot_buffers.check_tiling(owner, table)
                torch.cuda.synchronize()
                between_steps(c, guard, poison)
                values = []
                for step in range(2*c.nb_slots + 1):
                    ticket = c.submit(images)
                    r = check_step(ref, ticket, step)
                    values.append([r[key].tobytes() for key in sorted(r)] + [ticket.container()])
                    between_steps(c, guard, poison)
        seen[poison] = values
    assert seen[POISONS[0]] == seen[POISONS[1]]
