"""conv_gemm_split_kernel at the image borders: every lane loads the activations of its own position and marks the taps that
fall outside the image once per tile (csrc/hip/conv_gemm_split.hip, the activation loader). Small shapes whose tiles touch
each edge -- positions that are not a multiple of the 4 x 8 tile in either direction, images one tile row high, one tile,
one position -- against the CPU oracle, with the launch cut (tails finishing their heads' chains) and whole."""
import numpy
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, and a byte written outside a tensor fails the test (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF):
        yield


# (images, input height, input width)
CONV_SHAPES = [(2, 14, 46), (1, 6, 36), (3, 8, 16), (1, 2, 2), (2, 34, 70)]
TCONV_SHAPES = [(2, 5, 13), (1, 3, 5), (1, 1, 1), (2, 9, 17)]
FORMS = [('u', None), ('s', '1'), ('s', '3')]


def _vars(seed):
    from autoencoder_based_image_compression_amd.kodak.eae.graph import variables
    return variables.random_variables(1., False, seed=seed, bias_std=0.01)


def _run_forms(launch_options, call):
    outs = {}
    for (form, waves) in FORMS:
        launch_options.clear()
        launch_options.setenv('EAE_HIP_GEMM', form)
        if waves:
            launch_options.setenv('EAE_HIP_SPLIT_WAVES', waves)
        outs[(form, waves)] = call().cpu().numpy()
    launch_options.clear()
    return outs


@pytest.mark.parametrize('shape', CONV_SHAPES)
@pytest.mark.parametrize('norm', [0, 1])
def test_conv_edges_against_the_oracle(shape, norm, launch_options):
    from autoencoder_based_image_compression_amd import device as dev
    from oracle import transforms as orc
    v = _vars(41)
    x = numpy.random.RandomState(42).standard_normal(size=shape + (128,)).astype(numpy.float32)
    ref = orc.conv2d_same(x, v['encoder/weights_2'], 2, v['encoder/biases_2'])
    if norm:
        ref = orc.gdn(ref, v['encoder/gamma_2'], v['encoder/beta_2'])
    args = (torch.from_numpy(x).cuda(), dev.pack_conv_weights(torch.from_numpy(v['encoder/weights_2']).cuda()),
            torch.from_numpy(v['encoder/biases_2']).cuda(), norm, dev.pack_gamma(torch.from_numpy(v['encoder/gamma_2']).cuda()),
            torch.from_numpy(v['encoder/beta_2']).cuda())
    ws = dev.conv_workspace('cuda')
    for form, got in _run_forms(launch_options, lambda: dev.conv5x5s2(*args, workspace=ws)).items():
        assert numpy.array_equal(got, ref), form
    assert int(torch.count_nonzero(ws).item()) == 0


@pytest.mark.parametrize('shape', TCONV_SHAPES)
@pytest.mark.parametrize('norm', [0, 2])
def test_tconv_edges_against_the_oracle(shape, norm, launch_options):
    from autoencoder_based_image_compression_amd import device as dev
    from oracle import transforms as orc
    v = _vars(43)
    x = numpy.random.RandomState(44).standard_normal(size=shape + (128,)).astype(numpy.float32)
    ref = orc.conv2d_transpose_same(x, v['decoder/weights_4'], 2, v['decoder/biases_4'])
    if norm:
        ref = orc.gdn(ref, v['decoder/gamma_5'], v['decoder/beta_5'], inverse=True)
    args = (torch.from_numpy(x).cuda(), dev.pack_tconv_weights(torch.from_numpy(v['decoder/weights_4']).cuda()),
            torch.from_numpy(v['decoder/biases_4']).cuda(), norm, dev.pack_gamma(torch.from_numpy(v['decoder/gamma_5']).cuda()),
            torch.from_numpy(v['decoder/beta_5']).cuda())
    ws = dev.conv_workspace('cuda')
    for form, got in _run_forms(launch_options, lambda: dev.tconv5x5s2(*args, workspace=ws)).items():
        assert numpy.array_equal(got, ref), form
    assert int(torch.count_nonzero(ws).item()) == 0
