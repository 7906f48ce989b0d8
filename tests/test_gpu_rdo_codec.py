"""`codec.BatchCodec(..., rdo_lambda=...)` and `container.encode_images(..., rdo_lambda=...)`: the rate-distortion optimised quantiser
 through the pipelined codec and the container.

tests/test_gpu_quality_codec.py's inputs: three 176 x 208 images of different entropy (an 11 x 13 latent plane), `trained_like_variables`
with `decoder/weights_6` scaled, the tables of `stats.compute_binary_probabilities_ladder`. The rate point is 4 times the model's bin
widths and lambda is 0.01 (lambda / bw^2 = 0.25 bins^2 per bit). Chosen on the CPU, with the oracle's analysis transform and
`ratecontrol.rdo_quantize_numpy`, before this file was written: the rule then lowers 17.6 % of the non-zero nearest-rounded symbols of
the fixed model (17.3 % at L = 3) and 9.7 % of the learned one. Every case asserts that at least 1 % of them were lowered, on the
symbols the blobs hold, so none passes on an encoder that rounds to the nearest symbol.

Per case: `image_containers()` and `container()` equal `container.encode_images(..., rdo_lambda=lambda)` byte for byte;
`container.decode_images` of the blob and `codec.BatchDecoder` on it equal the ticket's reconstruction; 'sse' is that reconstruction's
squared error; the summed 'coder_bits' are those of the blob and below those of `rdo_lambda=None`. Launch by launch and replayed as
hipGraphs, with and without an exception map, the learned model, coding tiles of 4 x 4. Then `rdo_lambda=0.0` against today's bytes, and
the refusals. Every comparison is exact."""
import numpy
import pytest
import torch

import model_cases

pytestmark = pytest.mark.gpu

SHAPE = (176, 208)
BATCH = 3
MULTIPLIER = 4.
RDO_LAMBDA = 0.01
EXCEPTION = 5
MODES = {'launches': {}, 'graphs': {'use_graphs': True}}
# (model kind, truncated unary length, exception map, coding tile)
CASES = {'fixed_exception': (False, 10, EXCEPTION, None), 'fixed_no_exception': (False, 10, -1, None), 'learned_exception': (True, 10, EXCEPTION, None),
         'fixed_tiles_4x4': (False, 10, EXCEPTION, (4, 4)), 'fixed_L3': (False, 3, EXCEPTION, None)}
KEYS = ('nb_bits', 'coder_bits', 'exception_bits', 'sse', 'nb_deads', 'container_bytes')


def _images():
    """Noise, a noisy ramp and a nearly flat image: three different entropies."""
    rng = numpy.random.RandomState(2)
    (h, w) = SHAPE
    noise = rng.randint(16, 236, size=(h, w))
    ramp = numpy.clip(numpy.broadcast_to(16 + 219*numpy.arange(w)/(w - 1), (h, w)) + rng.randint(-4, 5, size=(h, w)), 16, 235)
    flat = rng.randint(16, 236, size=(h, w))//8 + 100
    return numpy.stack([noise, ramp, flat]).astype(numpy.uint8)


@pytest.fixture(scope='module')
def references():
    return {}


def _coder_bits(info, exception):
    per_map = info['nb_bits'].astype(numpy.int64).copy()
    if exception >= 0:
        per_map[:, exception] = 0                                # charged by its entropy (compression.py:68-81)
    return per_map.sum(axis=1)


def reference(cache, name):
    """Once per case, shared by the launch modes and the slots' module: the model, the rate point, and what `container.encode_images`
    and `container.decode_images` give with lambda, with 0.0 and without."""
    if name in cache:
        return cache[name]
    from autoencoder_based_image_compression_amd import container, pipeline
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables as var
    from autoencoder_based_image_compression_amd.kodak.lossless import stats as lossless_stats
    (learned, length, exception, tile) = CASES[name]
    v = model_cases.trained_like_variables(0.05, learned, seed=11 + int(learned))
    v['decoder/weights_6'] = (v['decoder/weights_6']*numpy.float32(30.)).astype(numpy.float32)
    encoder = pipeline.DeviceEncoder(v, learned)
    decoder = pipeline.DeviceDecoder(v, learned)
    images = _images()
    base = v[var.BIN_WIDTHS_NAME] if not learned else numpy.random.RandomState(17).uniform(0.04, 0.06, size=128).astype(numpy.float32)
    bin_widths = (numpy.float32(MULTIPLIER)*base).astype(numpy.float32)
    y = encoder(torch.from_numpy(images).cuda()).cpu().numpy()
    map_mean = lossless_stats.compute_map_mean(y)
    table = lossless_stats.compute_binary_probabilities_ladder(y, bin_widths[None], map_mean, length)[0]
    arguments = (encoder, bin_widths, map_mean, table, exception)
    more = {} if tile is None else {'coding_tile': tile}
    (blob, info) = container.encode_images(images, *arguments, rdo_lambda=RDO_LAMBDA, **more)
    (nearest_blob, nearest_info) = container.encode_images(images, *arguments, **more)
    decoded = container.decode_images(blob, decoder)
    difference = images.astype(numpy.int64) - decoded.astype(numpy.int64)
    # the symbols the two blobs hold: at least 1 % of the non-zero nearest-rounded ones were lowered, each by one, towards zero
    # (read out of the EAE1 blobs: the coding tile changes the streams, not the symbols)
    (whole, whole_nearest) = (blob, nearest_blob) if tile is None else (container.encode_images(images, *arguments, rdo_lambda=RDO_LAMBDA)[0],
                                                                       container.encode_images(images, *arguments)[0])
    symbols = container.decode_symbols(whole)[1].cpu().numpy().astype(numpy.int64)
    nearest = container.decode_symbols(whole_nearest)[1].cpu().numpy().astype(numpy.int64)
    moved = symbols != nearest
    share = moved.sum()/float((nearest != 0).sum())
    print(name, 'non-zero nearest-rounded symbols', int((nearest != 0).sum()), 'lowered', int(moved.sum()), 'share', share)
    assert share >= 0.01
    assert numpy.array_equal(symbols[moved], nearest[moved] - numpy.sign(nearest[moved]))
    assert numpy.abs(nearest[moved]).max() <= min(length, 16)
    if exception >= 0:
        assert not moved.reshape(BATCH, 128, -1)[:, exception].any()
    out = {'variables': v, 'learned': learned, 'length': length, 'exception': exception, 'tile': tile, 'images': images, 'bin_widths': bin_widths,
           'map_mean': map_mean, 'table': table, 'encoder': encoder, 'decoder': decoder, 'blob': blob, 'nearest_blob': nearest_blob,
           'image_blobs': [container.encode_images(images[i:i + 1], *arguments, rdo_lambda=RDO_LAMBDA, **more)[0] for i in range(BATCH)],
           'zero_blob': container.encode_images(images, *arguments, rdo_lambda=0., **more)[0], 'decoded': decoded,
           'sse': (difference*difference).sum(axis=(1, 2)), 'coder_bits': _coder_bits(info, exception),
           'nearest_coder_bits': _coder_bits(nearest_info, exception), 'payload_bytes': info['payload_bytes']}
    print(name, 'coder bits', out['coder_bits'].tolist(), 'with nearest rounding', out['nearest_coder_bits'].tolist(), 'sse', out['sse'].tolist())
    assert out['coder_bits'].sum() < out['nearest_coder_bits'].sum()
    assert out['zero_blob'] == nearest_blob and blob != nearest_blob
    cache[name] = out
    return out


def build(ref, mode, rdo_lambda=RDO_LAMBDA, **more):
    from autoencoder_based_image_compression_amd import codec
    if ref['tile'] is not None:
        more['coding_tile'] = ref['tile']
    return codec.BatchCodec(ref['variables'], ref['learned'], ref['bin_widths'], ref['map_mean'], ref['table'], ref['exception'], BATCH,
                            SHAPE[0], SHAPE[1], nb_in_flight=2, keep_reconstruction=True, emit_container=True, rdo_lambda=rdo_lambda,
                            **MODES[mode], **more)


def check_step(ref, ticket, step):
    """The ticket against `container.encode_images(..., rdo_lambda=...)` and `decode_images` of its blob."""
    r = ticket.result()
    assert set(r) == set(KEYS)                                    # `result()` gains no key
    assert ticket.image_containers() == ref['image_blobs'], step
    assert ticket.container() == ref['blob'], step
    assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), ref['decoded']), step
    assert numpy.array_equal(r['sse'], ref['sse']), step
    assert numpy.array_equal(r['coder_bits'], ref['coder_bits']), step
    assert int(r['coder_bits'].sum()) < int(ref['nearest_coder_bits'].sum()), step
    assert int(r['container_bytes'].sum()) == ref['payload_bytes'], step
    return r


@pytest.mark.parametrize('name, mode', [('fixed_exception', 'launches'), ('fixed_exception', 'graphs'), ('fixed_no_exception', 'launches'),
                                        ('learned_exception', 'launches'), ('fixed_tiles_4x4', 'launches'), ('fixed_tiles_4x4', 'graphs'),
                                        ('fixed_L3', 'launches')])
def test_codec_equals_encode_images_with_lambda(references, name, mode):
    from autoencoder_based_image_compression_amd import codec
    ref = reference(references, name)
    images = torch.from_numpy(ref['images']).cuda()
    with build(ref, mode) as c:
        assert c.rdo_lambda == RDO_LAMBDA
        tickets = [c.submit(images) for _ in range(c.nb_slots + 1)]
        for (step, ticket) in enumerate(tickets):
            check_step(ref, ticket, step)
        blob = tickets[-1].container()
    # the blob is an ordinary one: the resident decoder reads it as it reads any other
    more = {} if ref['tile'] is None else {'coding_tile': ref['tile']}
    with codec.BatchDecoder(ref['variables'], ref['learned'], BATCH, SHAPE[0], SHAPE[1], ref['length'], nb_in_flight=2, **more) as decoder:
        result = decoder.submit(blob).result()
        assert numpy.array_equal(result.cpu().numpy() if isinstance(result, torch.Tensor) else numpy.array(result), ref['decoded'])


def test_the_launches_of_a_step(references):
    """conv_3, gdn_3 as a launch of its own, the quantiser; the learned model skips gdn_3."""
    for (name, expected) in (('fixed_exception', ['conv1_gdn1', 'conv2_gdn2', 'conv3', 'gdn3', 'latent']),
                             ('learned_exception', ['conv1_gdn1', 'conv2_gdn2', 'conv3', 'latent'])):
        ref = reference(references, name)
        seen = []

        def hook(launch, fn):
            seen.append(launch)
            return fn()
        with build(ref, 'launches', launch_hook=hook) as c:
            check_step(ref, c.submit(torch.from_numpy(ref['images']).cuda()), 0)
        assert seen[:len(expected)] == expected and 'gdn3' not in seen[len(expected):] and seen.count('latent') == 1


@pytest.mark.parametrize('name, mode', [('fixed_exception', 'launches'), ('fixed_exception', 'graphs'), ('fixed_tiles_4x4', 'launches')])
def test_lambda_zero_gives_the_bytes_of_nearest_rounding(references, name, mode):
    ref = reference(references, name)
    images = torch.from_numpy(ref['images']).cuda()
    with build(ref, mode, rdo_lambda=0.) as c, build(ref, mode, rdo_lambda=None) as plain:
        (ticket, twin) = (c.submit(images), plain.submit(images))
        assert ticket.container() == twin.container() == ref['nearest_blob'] == ref['zero_blob']
        (r, t) = (ticket.result(), twin.result())
        for key in KEYS:
            assert numpy.array_equal(r[key], t[key]), key
        assert numpy.array_equal(ticket.reconstruction_uint8.cpu().numpy(), twin.reconstruction_uint8.cpu().numpy())


def test_refusals(references):
    from autoencoder_based_image_compression_amd import codec, ratecontrol
    ref = reference(references, 'fixed_exception')
    arguments = (ref['variables'], False, ref['bin_widths'], ref['map_mean'], ref['table'], EXCEPTION, BATCH, SHAPE[0], SHAPE[1])
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match='fuse_latent'):
        codec.BatchCodec(*arguments, fuse_latent=True, rdo_lambda=RDO_LAMBDA)
    with pytest.raises(ValueError, match='rdo_lambda'):
        codec.BatchCodec(*arguments, coder='host', rdo_lambda=RDO_LAMBDA)
    for value in (-1e-9, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='rdo_lambda'):
            codec.BatchCodec(*arguments, rdo_lambda=value)
        with pytest.raises(ValueError):
            ratecontrol.rdo_thresholds(ref['bin_widths'], ref['table'], value)
    ladder = ratecontrol.RateLadder(ref['bin_widths'][None], ref['table'][None], ref['map_mean'], EXCEPTION)
    head = (ref['variables'], False, ladder, BATCH, SHAPE[0], SHAPE[1])
    for value in (RDO_LAMBDA, 0.):
        with pytest.raises(ValueError, match='rdo_lambda'):
            codec.BudgetCodec(*head, budget_bytes=1 << 20, rdo_lambda=value)
        with pytest.raises(ValueError, match='rdo_lambda'):
            codec.TiledBudgetCodec(*head, (4, 4), budget_bytes=1 << 20, rdo_lambda=value)
        with pytest.raises(ValueError, match='rdo_lambda'):
            codec.QualityCodec(*head, target_psnr=30., rdo_lambda=value)
        with pytest.raises(ValueError, match='rdo_lambda'):
            codec.TiledQualityCodec(*head, (4, 4), target_psnr=30., rdo_lambda=value)
    assert torch.cuda.memory_allocated() == before                # refused in front of every allocation
    from autoencoder_based_image_compression_amd import container
    with pytest.raises(TypeError):
        container.encode_images_to_budget(ref['images'], ref['encoder'], ladder, 1 << 20, rdo_lambda=RDO_LAMBDA)
    with pytest.raises(TypeError):
        container.encode_images_to_quality(ref['images'], ref['encoder'], ref['decoder'], ladder, target_psnr=30., rdo_lambda=RDO_LAMBDA)
