"""Every leaf of the conv GEMM launch decision, at a size at which the launcher picks it BY ITSELF on one whole MI355X (256 CUs, 1,024
SIMDs), against the CPU oracle bit for bit.

The launcher (`launch()` and `try_split()` in csrc/hip/conv_gemm.hip, `launch_split()` in csrc/hip/conv_gemm_split.hip) chooses a kernel
form from the layer's shape and the number of CUs. The other GPU modules pin every form to the oracle by FORCING it onto shapes of a
few tiles (EAE_HIP_GEMM, EAE_HIP_FORCE_NT, EAE_HIP_PACK, EAE_HIP_SPLIT_WAVES); here each row of `CASES` is one layer call with default
launch options, declares the leaf it must land on, and the launcher's own record of what it launched (`device.last_gemm_plan`, the
test build's eae_hip_debug_last_gemm_plan: written beside the launch, not a second evaluation of the rules) is compared with that
declaration before the bits are compared with the oracle's. A threshold that moves, or grid arithmetic that changes behind one, fails
the plan assertion of the rows on either side of it.

TWO tile counts decide. `try_split()` counts the split kernel's tiles of 4 x 8 positions, s = n * ceil(hp/4) * ceil(wp/8) * phases,
and sends every layer with s >= 1024 to the split kernel; below that `launch()` counts the wave kernel's tiles of 8 x 4 positions,
w = n * ceil(hp/8) * ceil(wp/4) * phases, and compares THAT with the SIMDs (hp, wp: the positions the GEMM tiles -- half the input
size for the convolution, the input size and four phases for the transposed one). The two differ wherever hp is no multiple of 8 or
wp none of 4, so every row states both, a CPU test recomputes them from the shape, and the GPU test compares the launcher's count with
the row's. One consequence is a leaf of its own: a single-phase layer with s < 1024 <= w (132 x 248 positions: s = 1023, w = 1054)
reaches the clause `small_conv && items >= simds` of `launch()` and runs as half tiles even with a normalisation.

Every convolution row uses conv_3's weights and gdn_3's parameters from tests/model_cases.py (asymmetric gamma, one beta per channel), so
that the oracle's convolution of a shape is computed once and shared by the row without a normalisation, the row with one and the
eae_hip_conv5x5s2_latent rows of that shape. All comparisons are `numpy.array_equal`: the tolerance is zero, -0 == +0 the only slack."""
import collections

import numpy
import pytest
import torch

import model_cases
from test_gpu_kernels import _assert_handed_over


@pytest.fixture(autouse=True)
def guard():
    """Every test of this module runs on poisoned buffers between guard bands: what device.py / pipeline.py allocate holds 0xFF bytes
    (NaN, -1) until a kernel writes it, the inputs lie between bands as well (`guard.upload`), and a byte written outside a tensor
    fails the test (tests/guarded.py)."""
    import guarded
    from autoencoder_based_image_compression_amd import device, pipeline
    with guarded.guarded((device, pipeline), 0xFF) as g:
        yield g


SIMDS = 1024                 # one whole MI355X: 256 CUs x 4

# ---- the leaves, as the fields of device.last_gemm_plan() that name them ---------------------------------------------------------------
LEAVES = {
    'nt1 one-wave': {'family': 'wave', 'waves': 1, 'nt': 1, 'packed': 0, 'cut': 0},       # quarter tiles, one-wave blocks
    'nt1 packed': {'family': 'wave', 'waves': 4, 'nt': 1, 'packed': 1, 'cut': 0},         # quarter tiles, the four parts of a tile in one block
    'nt2 one-wave': {'family': 'wave', 'waves': 1, 'nt': 2, 'packed': 0, 'cut': 0},       # half tiles, one-wave blocks
    'nt2 packed': {'family': 'wave', 'waves': 4, 'nt': 2, 'packed': 1, 'cut': 0},         # half tiles, the parts of two tiles in one block
    'whole one-wave': {'family': 'wave', 'waves': 1, 'nt': 4, 'packed': 0, 'cut': 0},     # whole tiles, fused epilogue, one-wave blocks
    'split whole': {'family': 'split', 'waves': 4, 'nt': 4, 'packed': 0, 'cut': 0},       # one item per wave, nothing cut
    'split cut': {'family': 'split', 'waves': 4, 'nt': 4, 'packed': 0, 'cut': 1},         # the last tiles of every XCD's share cut in two
}

# Forms the library holds that NO launch with default options reaches on a whole MI355X, and why. They stay in the library: the
# parity tests of every form force them (tests/test_gpu_kernels.py: FORMS), and other devices or options select them.
UNREACHED = {
    'lds': 'the block-cooperative LDS form is launched for EAE_HIP_GEMM=l only',
    'two-wave blocks': 'launch() takes them from 65,536 positions on, i.e. from 2,048 tiles of 32 positions, and try_split() has sent every '
                       'layer of 1,024 tiles or more to the split kernel before (launch_split() declines only where the CUs are no multiple of 8)',
    'four-wave blocks of whole tiles': 'only EAE_HIP_FORCE_TILE=128 asks for them',
}


def _unreached_form(plan):
    """The name in UNREACHED of what `plan` records, or None."""
    if plan['family'] == 'lds':
        return 'lds'
    if plan['family'] == 'wave' and not plan['packed'] and plan['waves'] != 1:
        return 'two-wave blocks' if plan['waves'] == 2 else 'four-wave blocks of whole tiles'
    return None


# ---- the case table -------------------------------------------------------------------------------------------------------------------
# op: 'conv' (eae_hip_conv5x5s2[_ws], input 2hp x 2wp), 'tconv' (eae_hip_tconv5x5s2[_ws], input hp x wp), 'latent' (eae_hip_conv5x5s2_latent)
# norm: 0 / 1 (GDN) / 2 (IGDN); for 'latent': 'fixed' (gdn_3 and inverse_gdn_4 around the quantiser) or 'learned' (neither)
# s, w: the two tile counts of the module's docstring;  k: the resident waves per SIMD a cut is sized for, 0 where nothing is cut
# workspace: 'given', 'none' (workspace=False: the entry point without one) or 'partitioned' (EAE_HIP_ASSUME_PARTITIONED=1, a poisoned one)
Case = collections.namedtuple('Case', 'op n hp wp norm s w leaf k workspace')


def _case_id(c):
    return '{0}-{1}x{2}x{3}-{4}{5}'.format(c.op, c.n, c.hp, c.wp, {0: 'plain', 1: 'gdn', 2: 'igdn'}.get(c.norm, c.norm),
                                           '' if c.workspace == 'given' else '-' + c.workspace)


def _rows():
    rows = []

    def conv(n, hp, wp, s, w, with_norm, without, latent=None, extra=()):
        (leaf_n, k_n) = with_norm
        (leaf_0, k_0) = without
        rows.append(Case('conv', n, hp, wp, 0, s, w, leaf_0, k_0, 'given'))
        rows.append(Case('conv', n, hp, wp, 1, s, w, leaf_n, k_n, 'given'))
        for (workspace, leaf, k) in extra:
            rows.append(Case('conv', n, hp, wp, 1, s, w, leaf, k, workspace))
        if latent is not None:
            for mode in ('fixed', 'learned'):
                rows.append(Case('latent', n, hp, wp, mode, s, w, latent[0], latent[1], 'given'))

    def tconv(n, hp, wp, s, w, with_norm, without):
        rows.append(Case('tconv', n, hp, wp, 0, s, w, without[0], without[1], 'given'))
        rows.append(Case('tconv', n, hp, wp, 2, s, w, with_norm[0], with_norm[1], 'given'))

    # convolution, one image. w <= 256: quarter tiles; packed where a block per CU results (w = 256 exactly) and the width is a multiple of 4
    conv(1, 120, 68, 270, 255, ('nt1 one-wave', 0), ('nt1 one-wave', 0))
    conv(1, 64, 128, 256, 256, ('nt1 packed', 0), ('nt1 packed', 0))
    conv(1, 64, 126, 256, 256, ('nt1 one-wave', 0), ('nt1 one-wave', 0))            # width no multiple of 4
    # 256 < w <= 512: half tiles; packed at w = 512 where the width is a multiple of 8
    conv(1, 8, 1028, 258, 257, ('nt2 one-wave', 0), ('nt2 one-wave', 0))
    conv(1, 64, 256, 512, 512, ('nt2 packed', 0), ('nt2 packed', 0))
    conv(1, 64, 254, 512, 512, ('nt2 one-wave', 0), ('nt2 one-wave', 0))            # width no multiple of 8
    # 512 < w, s < 1024: whole tiles with the fused epilogue where a normalisation follows, half tiles (+ packed, width % 8 == 0) where none does
    conv(1, 216, 76, 540, 513, ('whole one-wave', 0), ('nt2 one-wave', 0))
    conv(1, 132, 128, 528, 544, ('whole one-wave', 0), ('nt2 packed', 0))
    conv(1, 372, 84, 1023, 987, ('whole one-wave', 0), ('nt2 one-wave', 0), latent=('nt2 one-wave', 0))      # latent: two launches
    # s = 1023 but w = 1054 >= 1024: the clause `small_conv && items >= simds` -- half tiles and a normalisation pass
    conv(1, 132, 248, 1023, 1054, ('nt2 packed', 0), ('nt2 packed', 0))
    # s >= 1024: the split kernel. Cut where ceil(s / 1024) * 1024 > 1.03 s, or s >= 3072; k = min(s // 1024, 3)
    conv(1, 128, 256, 1024, None, ('split whole', 0), ('split whole', 0), latent=('split whole', 0))        # one exact round
    conv(1, 100, 328, 1025, None, ('split cut', 1), ('split cut', 1), latent=('split cut', 1),
         extra=(('none', 'split whole', 0), ('partitioned', 'split whole', 0)))
    conv(1, 112, 568, 1988, None, ('split cut', 1), ('split cut', 1))                # 2048 > 1.03 x 1988 = 2047.6
    conv(1, 156, 408, 1989, None, ('split whole', 0), ('split whole', 0))            # 2048 < 1.03 x 1989 = 2048.7
    conv(1, 164, 400, 2050, None, ('split cut', 2), ('split cut', 2))
    conv(1, 168, 568, 2982, None, ('split cut', 2), ('split cut', 2))                # 3072 > 1.03 x 2982 = 3071.5
    conv(1, 76, 1256, 2983, None, ('split whole', 0), ('split whole', 0))            # 3072 < 1.03 x 2983 = 3072.5
    conv(1, 192, 512, 3072, None, ('split cut', 3), ('split cut', 3), latent=('split cut', 2))     # every tile cut; the latent instance holds two waves
    # conv_2 of two to five Kodak images
    conv(2, 64, 96, 384, 384, ('nt2 one-wave', 0), ('nt2 one-wave', 0))
    conv(3, 64, 96, 576, 576, ('whole one-wave', 0), ('nt2 packed', 0))
    conv(4, 64, 96, 768, 768, ('whole one-wave', 0), ('nt2 packed', 0))
    conv(5, 64, 96, 960, 960, ('whole one-wave', 0), ('nt2 packed', 0))
    # transposed convolution: four phases, so a quarter of the spatial tiles reaches each threshold
    tconv(1, 16, 128, 256, 256, ('nt1 packed', 0), ('nt1 packed', 0))
    tconv(1, 16, 126, 256, 256, ('nt1 one-wave', 0), ('nt1 one-wave', 0))
    tconv(1, 40, 52, 280, 260, ('nt2 one-wave', 0), ('nt2 one-wave', 0))
    tconv(1, 32, 128, 512, 512, ('nt2 packed', 0), ('nt2 packed', 0))
    tconv(1, 24, 172, 528, 516, ('whole one-wave', 0), ('nt2 one-wave', 0))
    tconv(1, 60, 132, 1020, 1056, ('whole one-wave', 0), ('nt2 one-wave', 0))        # w >= 1024 is nothing special with four phases
    tconv(1, 64, 128, 1024, None, ('split whole', 0), ('split whole', 0))            # four-phase launches are never cut by themselves
    # transpose_conv_1 of two to five Kodak images
    tconv(2, 32, 48, 384, 384, ('nt2 one-wave', 0), ('nt2 one-wave', 0))
    tconv(3, 32, 48, 576, 576, ('whole one-wave', 0), ('nt2 packed', 0))
    tconv(4, 32, 48, 768, 768, ('whole one-wave', 0), ('nt2 packed', 0))
    tconv(5, 32, 48, 960, 960, ('whole one-wave', 0), ('nt2 packed', 0))
    return rows


CASES = _rows()

# (op, normalised?, leaf, k) of every leaf a launch with default options reaches on a whole MI355X: the table must hold each of them.
REACHABLE = [
    ('conv', False, 'nt1 one-wave', 0), ('conv', True, 'nt1 one-wave', 0), ('conv', False, 'nt1 packed', 0), ('conv', True, 'nt1 packed', 0),
    ('conv', False, 'nt2 one-wave', 0), ('conv', True, 'nt2 one-wave', 0), ('conv', False, 'nt2 packed', 0), ('conv', True, 'nt2 packed', 0),
    ('conv', True, 'whole one-wave', 0),
    ('conv', False, 'split whole', 0), ('conv', True, 'split whole', 0),
    ('conv', False, 'split cut', 1), ('conv', True, 'split cut', 1), ('conv', False, 'split cut', 2), ('conv', True, 'split cut', 2),
    ('conv', False, 'split cut', 3), ('conv', True, 'split cut', 3),
    ('tconv', False, 'nt1 one-wave', 0), ('tconv', True, 'nt1 one-wave', 0), ('tconv', False, 'nt1 packed', 0), ('tconv', True, 'nt1 packed', 0),
    ('tconv', False, 'nt2 one-wave', 0), ('tconv', True, 'nt2 one-wave', 0), ('tconv', False, 'nt2 packed', 0), ('tconv', True, 'nt2 packed', 0),
    ('tconv', True, 'whole one-wave', 0),
    ('tconv', False, 'split whole', 0), ('tconv', True, 'split whole', 0),
    ('latent', True, 'nt2 one-wave', 0), ('latent', False, 'nt2 one-wave', 0),          # two launches: the convolution, then the stage
    ('latent', True, 'split whole', 0), ('latent', False, 'split whole', 0),
    ('latent', True, 'split cut', 1), ('latent', False, 'split cut', 1), ('latent', True, 'split cut', 2), ('latent', False, 'split cut', 2),
]

# The tile counts either side of every threshold, as (op, which count, value): a row with that count must be in the table.
BOUNDARIES = [
    ('conv', 'w', 255), ('conv', 'w', 256), ('conv', 'w', 257), ('conv', 'w', 512), ('conv', 'w', 513), ('conv', 'w', 1054),
    ('conv', 's', 1023), ('conv', 's', 1024), ('conv', 's', 1025), ('conv', 's', 1988), ('conv', 's', 1989), ('conv', 's', 2050),
    ('conv', 's', 2982), ('conv', 's', 2983), ('conv', 's', 3072),
    ('tconv', 'w', 256), ('tconv', 'w', 260), ('tconv', 'w', 512), ('tconv', 'w', 516), ('tconv', 's', 1020), ('tconv', 's', 1024),
    ('latent', 's', 1023), ('latent', 's', 1024), ('latent', 's', 1025), ('latent', 's', 3072),
]


def _phases(c):
    return 4 if c.op == 'tconv' else 1


def _ceil(a, b):
    return -(-a//b)


def _normalised(c):
    return c.norm in (1, 2, 'fixed')


# ---- CPU: the table itself --------------------------------------------------------------------------------------------------------------
def test_the_table_states_its_tile_counts_correctly():
    """s and w of every row are what the two launchers count for the row's shape; rows below 1,024 split-kernel tiles declare a wave-kernel
    leaf and state w, the others a split-kernel leaf; k goes with a cut and with nothing else."""
    assert len({_case_id(c) for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.s == c.n*_ceil(c.hp, 4)*_ceil(c.wp, 8)*_phases(c), c
        family = LEAVES[c.leaf]['family']
        if c.s < SIMDS:
            assert family == 'wave' and c.w == c.n*_ceil(c.hp, 8)*_ceil(c.wp, 4)*_phases(c), c
        else:
            assert family == 'split' and c.w is None, c
        assert (c.k in (1, 2, 3)) == (c.leaf == 'split cut'), c
        assert c.workspace in ('given', 'none', 'partitioned')
        assert c.n*(2*c.hp if c.op != 'tconv' else c.hp)*(2*c.wp if c.op != 'tconv' else c.wp)*128*4 < 256 << 20     # the guard bands an input this size


def test_the_table_holds_every_reachable_leaf_and_both_sides_of_every_threshold():
    """Deleting a row turns this red: every leaf a default launch reaches on a whole MI355X is declared by some row (no row declares
    anything else), and the tile counts either side of each threshold are present."""
    declared = {(c.op, _normalised(c), c.leaf, c.k) for c in CASES if c.workspace == 'given'}
    assert declared == set(REACHABLE), (sorted(declared - set(REACHABLE)), sorted(set(REACHABLE) - declared))
    assert len(REACHABLE) == len(set(REACHABLE))
    for (op, which, value) in BOUNDARIES:
        assert any(c.op == op and getattr(c, which) == value for c in CASES), (op, which, value)
    for op in ('conv', 'tconv'):                                       # the batches a user sends: two to five Kodak images
        (hp, wp) = (64, 96) if op == 'conv' else (32, 48)
        assert {c.n for c in CASES if c.op == op and (c.hp, c.wp) == (hp, wp)} == {2, 3, 4, 5}
    for c in CASES:                                                    # each layer with its normalisation and without
        if c.op != 'latent' and c.workspace == 'given':
            assert {d.norm for d in CASES if (d.op, d.n, d.hp, d.wp) == (c.op, c.n, c.hp, c.wp)} == ({0, 1} if c.op == 'conv' else {0, 2}), c
        if c.op == 'latent':
            assert {d.norm for d in CASES if d.op == 'latent' and (d.n, d.hp, d.wp) == (c.n, c.hp, c.wp)} == {'fixed', 'learned'}
    assert {c.workspace for c in CASES if c.leaf == 'split whole' and c.s == 1025} == {'none', 'partitioned'}


def test_no_row_declares_a_form_that_default_launches_do_not_reach():
    """UNREACHED names the forms, each with its reason; no leaf of the table records as one of them (the GPU test asserts the same of
    every recorded plan)."""
    assert all(reason.strip() for reason in UNREACHED.values())
    assert {_unreached_form(dict(LEAVES[c.leaf])) for c in CASES} == {None}
    probes = ({'family': 'lds', 'waves': 4, 'packed': 0}, {'family': 'wave', 'waves': 2, 'packed': 0}, {'family': 'wave', 'waves': 4, 'packed': 0})
    assert {_unreached_form(p) for p in probes} == set(UNREACHED)
    assert _unreached_form({'family': 'wave', 'waves': 4, 'packed': 1}) is None


# ---- what a row expects of the launcher's record -----------------------------------------------------------------------------------------
def _expected_plan(c):
    """The declared leaf as the full record. grid: the launchers' block counts restated -- wave kernel: the tiles padded to a multiple
    of 8 (one contiguous share per XCD), times phases, times the 4 / nt channel parts where those are blocks of their own; packed:
    blocks of nt position tiles, 4 nt columns wide; split kernel: four items per block, 8 interleaved shares of ceil(spatial / 8) x
    phases items plus, where the launch is cut, one tail per cut tile (at most 32 CUs x 4 SIMDs x k per XCD)."""
    plan = dict(LEAVES[c.leaf])
    phases = _phases(c)
    plan['k'] = c.k
    plan['block'] = 64*plan['waves']
    norm = c.norm if c.op != 'latent' else 0
    plan['norm_pass'] = 1 if (plan['nt'] < 4 and norm) else 0
    if c.op == 'latent':
        plan['latent_fused'] = 1 if plan['family'] == 'split' else 0
    else:
        plan['latent_fused'] = -1
    if plan['family'] == 'split':
        plan['items'] = c.s
        share = _ceil(c.s//phases, 8)*phases
        tails = min(share, 32*4*c.k) if plan['cut'] else 0
        plan['grid'] = _ceil(share + tails, 4)*8
    else:
        plan['items'] = c.w
        if plan['packed']:
            assert c.wp % (4*plan['nt']) == 0
            plan['grid'] = _ceil(c.n*_ceil(c.hp, 8)*(c.wp//(4*plan['nt'])), 8)*8*phases
        else:
            plan['grid'] = _ceil(c.w//phases, 8)*8*phases*(4//plan['nt'])
    return plan


def test_expected_grids_of_some_rows_by_hand():
    by_id = {_case_id(c): c for c in CASES}
    assert _expected_plan(by_id['conv-1x100x328-gdn'])['grid'] == 520           # 129 items per share + 128 tails = 257 waves -> 65 blocks x 8
    assert _expected_plan(by_id['conv-1x128x256-plain'])['grid'] == 256         # 128 items per share, four to a block
    assert _expected_plan(by_id['conv-1x192x512-gdn'])['grid'] == 1536          # 384 + 384 tails -> 192 blocks x 8
    assert _expected_plan(by_id['latent-1x192x512-fixed'])['grid'] == 1280      # 384 + 256 tails -> 160 blocks x 8
    assert _expected_plan(by_id['conv-1x64x128-gdn'])['grid'] == 256            # one four-wave block per tile and CU
    assert _expected_plan(by_id['conv-1x120x68-plain'])['grid'] == 1024         # 255 tiles -> 256, four quarter blocks each
    assert _expected_plan(by_id['tconv-1x40x52-igdn'])['grid'] == 576           # 65 tiles -> 72, four phases, two half blocks each
    assert _expected_plan(by_id['tconv-3x32x48-plain'])['grid'] == 288          # 3 x 4 x 6 blocks of two tiles = 72, four phases
    assert _expected_plan(by_id['tconv-1x64x128-igdn'])['grid'] == 256


# ---- GPU: every row -------------------------------------------------------------------------------------------------------------------
_shared = {}


def _once(key, make):
    """The oracle's convolution of ONE shape at a time (the table keeps the rows of a shape together): computed once, shared by the
    rows that need it, never written to; the previous shape's arrays are dropped."""
    if _shared.get('key') != key:
        _shared.clear()
        _shared.update(key=key, value=make())
    return _shared['value']


_model = {}


def _variables():
    if not _model:
        _model.update(model_cases.trained_like_variables(1., False, seed=71))
    return _model


def _conv_reference(c):
    from oracle import transforms as orc
    v = _variables()
    x = numpy.random.default_rng([72, c.n, c.hp, c.wp]).standard_normal(size=(c.n, 2*c.hp, 2*c.wp, 128), dtype=numpy.float32)
    return (x, orc.conv2d_same(x, v['encoder/weights_3'], 2, v['encoder/biases_3']))


def _tconv_reference(c):
    from oracle import transforms as orc
    v = _variables()
    x = numpy.random.default_rng([73, c.n, c.hp, c.wp]).standard_normal(size=(c.n, c.hp, c.wp, 128), dtype=numpy.float32)
    return (x, orc.conv2d_transpose_same(x, v['decoder/weights_4'], 2, v['decoder/biases_4']))


def _host(t):
    return t.cpu().numpy()


def _workspace(c, dev, launch_options):
    if c.workspace == 'none':
        return False
    if c.workspace == 'partitioned':
        launch_options.setenv('EAE_HIP_ASSUME_PARTITIONED', '1')
        assert not dev.partition_info()['whole_device']
        return torch.full_like(dev.conv_workspace('cuda'), 0x5a5a5a5a)      # a cut launch would read its flags out of this
    return dev.conv_workspace('cuda')


def _assert_workspace(c, dev, ws):
    if c.workspace == 'given':
        _assert_handed_over(torch, dev, ws)
    elif c.workspace == 'partitioned':
        assert bool((ws == 0x5a5a5a5a).all())                               # left untouched


def _assert_plan(c, dev):
    plan = dev.last_gemm_plan()
    print('{0}: s = {1}, w = {2}, recorded {3}'.format(_case_id(c), c.s, c.w, plan))
    assert _unreached_form(plan) is None, (UNREACHED[_unreached_form(plan)], plan)
    assert plan == _expected_plan(c), (c, plan, _expected_plan(c))


def _latent_row(c, guard, dev, launch_options):
    from oracle import transforms as orc
    v = _variables()
    (x, raw) = _once(('conv', c.n, c.hp, c.wp), lambda: _conv_reference(c))
    rng = numpy.random.RandomState(74)
    bw = rng.uniform(0.05, 0.5, size=128).astype(numpy.float32)
    mean = rng.normal(scale=0.05, size=128).astype(numpy.float32)
    fixed = c.norm == 'fixed'
    y = orc.gdn(raw, v['encoder/gamma_3'], v['encoder/beta_3']) if fixed else raw
    q = model_cases.quantize(y, bw, mean)
    t = orc.gdn(q['shifted'], v['decoder/gamma_4'], v['decoder/beta_4'], inverse=True) if fixed else None
    gdn_in = (dev.pack_gamma(guard.upload(v['encoder/gamma_3'])), guard.upload(v['encoder/beta_3'])) if fixed else None
    igdn_out = (dev.pack_gamma(guard.upload(v['decoder/gamma_4'])), guard.upload(v['decoder/beta_4'])) if fixed else None
    ws = _workspace(c, dev, launch_options)
    got = dev.conv5x5s2_latent(guard.upload(x), dev.pack_conv_weights(guard.upload(v['encoder/weights_3'])), guard.upload(v['encoder/biases_3']),
                               guard.upload(bw), guard.upload(mean), gdn_in=gdn_in, igdn_out=igdn_out, want_y=True, want_shifted=True,
                               want_flags=True, workspace=ws)
    _assert_plan(c, dev)
    for (key, ref) in (('y', y), ('shifted', q['shifted']), ('symbols', q['symbols']), ('nonzero_flags', q['nonzero_flags'])):
        assert numpy.array_equal(_host(got[key]).reshape(ref.shape), ref), key
    assert got['checks'].cpu().tolist() == q['checks']
    if fixed:
        assert numpy.array_equal(_host(got['t']), t)
    else:
        assert got['t'] is None
    assert int(numpy.abs(q['symbols']).max()) > 2 and q['checks'][0] == 0      # the quantiser is exercised, nothing out of range
    _assert_workspace(c, dev, ws)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_a_default_launch_lands_on_its_leaf_and_gives_the_oracles_bits(c, guard, launch_options):
    """(a) the launcher's record equals the declared leaf, k, grid and block; (b) the output equals the oracle's; (c) a workspace that
    was given is handed back all zero with nothing to collect (a poisoned one of a launch that must not cut: untouched); (d) the
    guard bands of every buffer are intact."""
    from autoencoder_based_image_compression_amd import device as dev
    from oracle import transforms as orc
    launch_options.clear()
    assert dev.partition_info() == {'compute_units': 256, 'xcds': 8, 'whole_device': True}      # the leaves are those of one whole MI355X
    v = _variables()
    if c.op == 'latent':
        _latent_row(c, guard, dev, launch_options)
    else:
        if c.op == 'conv':
            (x, raw) = _once(('conv', c.n, c.hp, c.wp), lambda: _conv_reference(c))
            (w, bias, gamma, beta) = (dev.pack_conv_weights(guard.upload(v['encoder/weights_3'])), v['encoder/biases_3'], v['encoder/gamma_3'], v['encoder/beta_3'])
            call = dev.conv5x5s2
        else:
            (x, raw) = _once(('tconv', c.n, c.hp, c.wp), lambda: _tconv_reference(c))
            (w, bias, gamma, beta) = (dev.pack_tconv_weights(guard.upload(v['decoder/weights_4'])), v['decoder/biases_4'], v['decoder/gamma_5'], v['decoder/beta_5'])
            call = dev.tconv5x5s2
        ref = orc.gdn(raw, gamma, beta, inverse=c.norm == 2) if c.norm else raw
        ws = _workspace(c, dev, launch_options)
        got = call(guard.upload(x), w, guard.upload(bias), c.norm, dev.pack_gamma(guard.upload(gamma)), guard.upload(beta), workspace=ws)
        _assert_plan(c, dev)
        got = _host(got)
        assert got.shape == ref.shape and numpy.array_equal(got, ref)
        _assert_workspace(c, dev, ws)
    guard.check()
