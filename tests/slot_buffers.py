"""What every buffer of a resident codec's slot may hold when a step starts (a plain helper module: import it, no fixture lives here).

`codec.BatchCodec` makes its buffers once (`codec._Slot`), and so do the three resident decoders -- `codec.BatchDecoder`,
`BatchDecoder(coding_tile=...)` and `codec.RegionDecoder` --, which share ONE lane and ONE slot class (`codec._DecodeLane`,
`codec._DecodeSlot`); they reuse them step after step. A step that reads what the previous step left usually finds plausible data --
most tests leave the same data --, so tests/test_gpu_codec_slots.py and tests/test_gpu_region_decoder.py fill, between two steps, every
buffer a step must not depend on with a poison byte. Which buffers those are is decided HERE, attribute by attribute, from the
source; tests/test_slot_inventory.py keeps the three tables complete.

SCRATCH       a step defines all of it that it later reads, before reading it: it may hold anything when the step starts. Pinned
              buffers count on both sides: the device defines what the host reads, the host (`plan_decode_step`, `submit`) what the
              device reads.
CARRIED       a step expects a defined state left by construction or by the previous step, and restores it.
CONSTANT      written at construction, only read afterwards.
CONTAINER     an allocation whose bytes are covered entirely by classified parts (`check_tiling` asserts it on the live object).
NOT_A_BUFFER  events, counters' Python sides, host numpy views of a classified pinned tensor, streams, graph objects.

An entry is `name: Entry(class, reason, ...)`; the reason names the line it rests on (codec.py, device.py or a .hip file of
csrc/hip, as of the commit that last touched the entry). Tuples, lists and helper objects are classified through their members:
`coder_streams.streams`, `classes[].offsets`, `graphs[1]`. `alias`: the entry is a view of another entry's bytes and is poisoned
through that one. `get`: how the member's tensors are reached on a live object (default: the attribute itself).
"""
import collections

import torch

SCRATCH, CARRIED, CONSTANT, CONTAINER, NOT_A_BUFFER = ('SCRATCH', 'CARRIED', 'CONSTANT', 'CONTAINER', 'NOT_A_BUFFER')
CLASSES = (SCRATCH, CARRIED, CONSTANT, CONTAINER, NOT_A_BUFFER)

Entry = collections.namedtuple('Entry', ('cls', 'reason', 'get', 'parts', 'alias', 'max_gap'))


def _entry(cls, reason, get=None, parts=None, alias=None, max_gap=0):
    return Entry(cls, reason, get, parts, alias, max_gap)


def _streams_of(owner):
    """The `device.CoderStreams` of a slot or lane: the one of whole maps, or one per shape class of coding tiles."""
    if getattr(owner, 'coder_streams', None) is not None:
        return [owner.coder_streams]
    return [entry[0] for entry in (getattr(owner, 'classes', None) or [])]


def _graph_member(position):
    return lambda slot: [slot.graphs[position]] if slot.graphs is not None else []


_RESULT_ROWS = ('`CoderStreams.results` and its rows `.bac_bits`, `.bypass_bits`, `.status`, `.stage` are views of the results block the '
                'slot passes in (device.py:628, 632; codec.py:667, 622 / 1637, 622)')
_RESULT_ROW = 'a row of `CoderStreams.results` (device.py:632), itself a view of the slot\'s results block'


def _result_rows(prefix):
    """The four rows a `device.CoderStreams` unbinds from its results (device.py:632), as aliases of the slot's `results`."""
    return {prefix + '.' + row: _entry(SCRATCH, _RESULT_ROW, alias='results') for row in ('bac_bits', 'bypass_bits', 'status', 'stage')}


# ---- codec._Slot: one step in flight of BatchCodec ------------------------------------------------------------------------------
SLOT = {
    'block': _entry(CONTAINER, 'codec.py:634: [out | sse]; `out` is cut into the five blocks below (codec.py:629)',
                    parts=('results', 'hist', 'overflow', 'flags', 'checks', 'sse')),
    'out': _entry(CONTAINER, 'codec.py:635: block[:nb_words], cut by `cut` (codec.py:629)', parts=('results', 'hist', 'overflow', 'flags', 'checks')),
    'results': _entry(SCRATCH, 'coder_simd.hip:176, 234-238: binarise_kernel writes both bit counts, status and stage of EVERY map, '
                               'the ones with prob_row < 0 too, before any reader; coder="none" zeroes them (codec.py:1217); with '
                               'coder="host" the worker replaces what it read by zeros (codec.py:447)'),
    'hist': _entry(CARRIED, 'symbol_histograms(zero=False) adds into it (codec.py:1168); zeroed at construction (codec.py:634) and by '
                            'the coder side\'s publish_step from clear_from = 4*n_streams on (codec.py:1204, 1225; misc.hip:128)'),
    'overflow': _entry(CARRIED, 'as `hist`: the same kernel adds, the same publish_step clears (codec.py:1168, 1225)'),
    'flags': _entry(CARRIED, 'the latent stage only sets (device.py:349); cleared by the coder side\'s publish_step (codec.py:1225)'),
    'checks': _entry(CARRIED, 'the latent stage only adds (device.py:349; codec.py:1160, 1166); cleared by publish_step (codec.py:1225); its '
                              'fourth word is never touched'),
    'sse': _entry(CARRIED, 'tconv9x9s4_luma adds the squared errors (codec.py:1243); the synthesis side\'s publish_step clears from 0 on '
                           '(codec.py:1246)'),
    'unfinished': _entry(CARRIED, 'the low half of sse[batch_size] (codec.py:638): publish_step adds the conv workspace\'s error word '
                                  '(misc.hip:121) and clears it with the rest of `sse` (misc.hip:128)', alias='sse'),
    'pinned_out': _entry(SCRATCH, 'publish_step copies ALL of `out` in front of the step counter the host waits for (misc.hip:127, 139)'),
    'pinned_sse': _entry(SCRATCH, 'publish_step copies all of `sse` in front of the synthesis side\'s counter (codec.py:1246; misc.hip:127)'),
    'host_views': _entry(NOT_A_BUFFER, 'numpy views of pinned_out and pinned_sse (codec.py:642)'),
    'symbols': _entry(SCRATCH, 'the latent stage writes every symbol of every map (codec.py:1159, 1166; out_symbols holds N x C x hw)'),
    'symbols_2d': _entry(SCRATCH, 'a view of `symbols` (codec.py:644)', alias='symbols'),
    'gathered': _entry(SCRATCH, 'tile_symbols_gather writes every tile of the plan (codec.py:1193); the pad between two class runs is '
                                'never read (the classes\' views end at n*size, codec.py:663); with one tile it IS `symbols` (codec.py:657)'),
    'classes': _entry(NOT_A_BUFFER, 'a list of tuples; its members are the entries `classes[]...` below (codec.py:679, 623)'),
    'classes[].streams': _entry(SCRATCH, 'as `coder_streams.streams`, per shape class (codec.py:622)',
                                get=lambda slot: [s.streams for s in _streams_of(slot)] if slot.coder_streams is None else []),
    'classes[].results': _entry(SCRATCH, _RESULT_ROWS, alias='results'),
    'classes[].tiles': _entry(SCRATCH, 'views of `gathered` (codec.py:679, 623)', alias='gathered'),
    'classes[].rows': _entry(CONSTANT, 'views of the CODEC\'s `_tile_prob_row`, uploaded once (codec.py:868, 679): not the slot\'s bytes'),
    'classes[].offsets': _entry(SCRATCH, 'views of `offsets` (codec.py:679, 624)', alias='offsets'),
    'coder_streams': _entry(NOT_A_BUFFER, 'a device.CoderStreams (codec.py:647; None with coding tiles); its members are the two entries below'),
    'coder_streams.streams': _entry(SCRATCH, 'binarise_kernel writes the bypass words it counts (coder_simd.hip:227, 233), emit_kernel the '
                                             'arithmetic-coded words as whole words; the decoder core loads 16-byte groups that hold stream '
                                             'bits only (coder_simd.hip:585) and takes no bit beyond them (`left`); the pack copies the '
                                             'counted bytes (container.hip:24-30). (The chunked round trip of coder_chunks > 1, experimental '
                                             'build only, is out of scope: see `workspace`.)',
                                    get=lambda slot: [slot.coder_streams.streams] if slot.coder_streams is not None else []),
    'coder_streams.results': _entry(SCRATCH, _RESULT_ROWS, alias='results'),
    'workspace': _entry(SCRATCH, 'binarise_kernel writes ndec and the decisions it counts (coder_simd.hip:214, 234), the encoder core masks '
                                 'the bytes beyond them (coder_simd.hip:301-305) and writes the records emit_kernel reads (masked at '
                                 'coder_simd.hip:406); the decoder core only WRITES prefixes (coder_simd.hip:695, 740), debinarise_kernel '
                                 'resets ndec before compare_kernel reads it (coder_simd.hip:785, 911). Out of scope: with coder_chunks > 1 '
                                 '(codec.py:648; the experimental build only, device.py:783) it is a coder_trailing_workspace whose dec_state / '
                                 'avail_bits are filled at the head of every call (coder_simd.hip:1591-1592); no case runs that form poisoned'),
    'conv_ws': _entry(CARRIED, 'the split conv GEMM polls its flags: every launch leaves it zeroed (device.py:218), publish_step restores it '
                               'after a failed hand-over (misc.hip:120)'),
    'seq_dev': _entry(CARRIED, 'step counters and publish_step\'s ticket words (codec.py:671; misc.hip:133-138)'),
    'pinned_seq': _entry(CARRIED, 'the published counters the worker compares with `counts` (codec.py:672, 985)'),
    'seq_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_seq (codec.py:673)'),
    'coder_seq': _entry(CARRIED, 'views of seq_dev and pinned_seq (codec.py:675)', alias='seq_dev'),
    'synthesis_seq': _entry(CARRIED, 'views of seq_dev and pinned_seq (codec.py:676)', alias='seq_dev'),
    'counts': _entry(CARRIED, 'how many times the host has submitted each side (codec.py:677, 988): a Python list, no device bytes'),
    'free': _entry(NOT_A_BUFFER, 'a threading.Event (codec.py:678)'),
    'pinned_symbols': _entry(SCRATCH, 'coder="host": one copy of all of `symbols` per step (codec.py:1215)'),
    'staging': _entry(SCRATCH, 'a host batch is copied over all of it before the first kernel (codec.py:1086-1087, 954)'),
    'pinned_rec': _entry(SCRATCH, 'the worker copies the whole reconstruction (codec.py:432)'),
    'graphs': _entry(NOT_A_BUFFER, '(graph objects, static input, latents, reconstruction) (codec.py:1064, 1075): the three tensors are the '
                                   'entries `graphs[1..3]` below; what else a capture allocates cannot be reached from here'),
    'graphs[0]': _entry(NOT_A_BUFFER, 'the torch.cuda.CUDAGraph objects (codec.py:1059, 1066)'),
    'graphs[1]': _entry(SCRATCH, 'the static input: every replay copies the step\'s batch over all of it first (codec.py:1011, 1014)', get=_graph_member(1)),
    'graphs[2]': _entry(SCRATCH, 'the synthesis side\'s input: written by the captured latent stage / tconv1 of graphs[0] on every replay, '
                                 'read by graphs[2] (codec.py:1068-1074)', get=_graph_member(2)),
    'graphs[3]': _entry(SCRATCH, 'the reconstruction: tconv9x9s4_luma writes every pixel on every replay (codec.py:1242)', get=_graph_member(3)),
    'table': _entry(CONTAINER, 'codec.py:692: [the codec\'s rows | one row per image]', parts=('table[:nb_maps]', 'exception_rows')),
    'table[:nb_maps]': _entry(CONSTANT, 'the codec\'s probability rows, copied at construction (codec.py:693) and only read by the coder',
                              get=lambda slot: [slot.table[:slot.table.shape[0] - slot.exception_rows.shape[0]]] if slot.emit_host is not None else []),
    'exception_rows': _entry(SCRATCH, 'with an exception map exception_rows_kernel writes all L entries of every image\'s row in front of the '
                                      'coder (codec.py:1187; codec_container.hip:218); without one no prob_row names them (codec.py:826-828) and '
                                      'the worker takes none (codec.py:487)'),
    'index': _entry(SCRATCH, 'index_streams_kernel / index_entry_bases_kernel write every word (codec_container.hip:73-77, 160-164) in front '
                             'of pack and publish'),
    'payload_bytes': _entry(SCRATCH, 'index[0:1] (codec.py:696)', alias='index'),
    'offsets': _entry(SCRATCH, 'index_streams_kernel writes every entry (codec_container.hip:63); in tiles index_entry_pieces_kernel writes '
                               'every piece of every entry, the first too (codec_container.hip:120, 124), before index_entry_bases_kernel '
                               'reads the first pieces'),
    'payload': _entry(SCRATCH, 'the pack writes [0, payload bytes); publish_prefix copies that prefix rounded up to 16 (codec_container.hip:'
                               '185-189) and the worker takes payload[:payload_bytes] (codec.py:489)'),
    'pinned_payload': _entry(SCRATCH, 'as `payload`: the host reads the announced prefix only, and none of it when the overflow flag is set (codec.py:489)'),
    'emit_tail': _entry(CONTAINER, 'codec.py:697: [exception rows | index words], published as one', parts=('exception_rows', 'index')),
    'pinned_emit': _entry(SCRATCH, 'publish_to_host copies all of emit_tail in front of the step counter (codec.py:1203, 1224)'),
    'emit_host': _entry(NOT_A_BUFFER, 'the container\'s fixed parts, the capacity, and numpy views of pinned_payload and pinned_emit (codec.py:704)'),
}

# ---- codec._DecodeLane: the device side of one slot of BatchDecoder, BatchDecoder(coding_tile=...) and RegionDecoder --------------
_HEAD = ('a field of `head`: fetch_prefix copies head_bytes = ALL of the pinned head first (codec.py:1876), and plan_decode_step has written '
         'every element of every field (codec.py:1418-1442), plan_region_step of a RegionDecoder\'s (codec.py:2156-2173)')
_REGION_HEAD = ('a field of a RegionDecoder\'s `head` (codec.py:1621; None otherwise): fetch_prefix copies ALL of the pinned head first '
                '(codec.py:1876), and plan_region_step has written every element ')
DECODE_LANE = {
    'stream': _entry(NOT_A_BUFFER, 'the stream the lane\'s steps run on (codec.py:1609)'),
    'head': _entry(CONTAINER, 'codec.py:1611: the fields of the decoder\'s head (decode_head_layout, region_head_layout), each on an 8-byte '
                              'boundary, the block rounded up to 16 (codec.py:1306-1309)',
                   parts=('head_bits', 'prob_row', 'placement', 'crop_origin', 'bin_widths', 'map_mean', 'table', 'payload_bytes'), max_gap=15),
    'head_bits': _entry(SCRATCH, _HEAD),
    'prob_row': _entry(SCRATCH, _HEAD),
    'placement': _entry(SCRATCH, _REGION_HEAD + '(codec.py:2158, 2164)'),
    'crop_origin': _entry(SCRATCH, _REGION_HEAD + '(codec.py:2159, 2165)'),
    'bin_widths': _entry(SCRATCH, _HEAD),
    'map_mean': _entry(SCRATCH, _HEAD),
    'table': _entry(SCRATCH, _HEAD),
    'payload_bytes': _entry(SCRATCH, _HEAD + '; fetch_prefix and the index clamp what it announces to the capacity (codec_decode.hip:17)'),
    'head_bytes': _entry(CONSTANT, 'the size of the head, written at construction (codec.py:1627), read by fetch_prefix'),
    'payload': _entry(SCRATCH, 'fetch_prefix copies the announced bytes (codec.py:1877); the unpack reads inside them (container.hip:27-30)'),
    'status': _entry(CONTAINER, 'codec.py:1631: [results | index words]', parts=('results', 'index')),
    'results': _entry(SCRATCH, 'rows 0-1: copied from head_bits (codec.py:1878); row 2: eae_hip_coder_decode_batch fills it with zeros '
                               '(coder_simd.hip:1478); row 3 (stage) is written with every non-zero status (coder_device.hip:246-247) and '
                               'read by the worker only next to one (codec.py:1542)'),
    'index': _entry(SCRATCH, 'as `_Slot.index`: every word written by the index kernels (codec.py:1897, 1905, 2246)'),
    'offsets': _entry(SCRATCH, 'as `_Slot.offsets` (codec.py:1897, 1905, 2246), in front of the unpack'),
    'coder_streams': _entry(NOT_A_BUFFER, 'a device.CoderStreams (codec.py:1637; None for a step in tiles); its members are the two entries below'),
    'coder_streams.streams': _entry(SCRATCH, 'the unpack writes the counted bytes of every piece (container.hip:24-30); the decoder core '
                                             'loads 16-byte groups that hold stream bits only and takes none beyond them (coder_simd.hip:585, '
                                             '610); debinarise_kernel masks the bypass words beyond the count (coder_simd.hip:821, 854)',
                                    get=lambda lane: [lane.coder_streams.streams] if lane.coder_streams is not None else []),
    'coder_streams.results': _entry(SCRATCH, _RESULT_ROWS, alias='results'),
    'workspace': _entry(SCRATCH, 'the decoder core writes the prefix bytes debinarise_kernel reads (coder_simd.hip:695, 740), debinarise_kernel '
                                 'or mark_kernel writes ndec (coder_simd.hip:785, 1387); nothing is read first'),
    'symbols': _entry(SCRATCH, 'debinarise_kernel (or the general kernel) writes every symbol of every coded map (coder_simd.hip:896). The maps '
                               'of an ABSENT image (prob_row -1) are left as they are and dequantised with bin width 0 and mean 0 '
                               '(codec.py:1439-1440) into planes no ticket returns (codec.py:1694)'),
    'decoded': _entry(SCRATCH, 'as `symbols`, tile-major (codec.py:1907-1908, 2248-2250); the pad between two class runs is never read, and '
                               'an absent slot of a RegionDecoder (placement -1, codec.py:2158) is not placed'),
    'classes': _entry(NOT_A_BUFFER, 'a list of tuples (None for whole maps); its members are the entries `classes[]...` below (codec.py:1644, 623)'),
    'classes[].streams': _entry(SCRATCH, 'as `coder_streams.streams`, per shape class (codec.py:622)',
                                get=lambda lane: [s.streams for s in _streams_of(lane)] if lane.coder_streams is None else []),
    'classes[].results': _entry(SCRATCH, _RESULT_ROWS, alias='results'),
    'classes[].tiles': _entry(SCRATCH, 'views of `decoded` (codec.py:1644, 623)', alias='decoded'),
    'classes[].rows': _entry(SCRATCH, 'views of `prob_row` (codec.py:1644, 623)', alias='prob_row'),
    'classes[].offsets': _entry(SCRATCH, 'views of `offsets` (codec.py:1644, 624)', alias='offsets'),
    'shifted': _entry(SCRATCH, 'the dequantiser writes every latent of every image (codec.py:1900, 1908: every latent is in one tile) and of '
                               'every PRESENT crop\'s window (codec.py:2250); the window of an absent crop is synthesised as it is, into planes '
                               'no crop is cut from for a ticket (codec.py:1697)'),
    'scratch': _entry(SCRATCH, 'eae_hip_decode zeroes its conv workspace and status word itself, by a kernel, at the head of every call '
                               '(model.hip:199); the activations are written before they are read'),
    'unfinished': _entry(SCRATCH, 'the status word inside `scratch` (device.py:191)', alias='scratch'),
}

# ---- codec._DecodeSlot: what one step in flight of the three resident decoders owns beside its lane -------------------------------
DECODE_SLOT = {
    'lane': _entry(NOT_A_BUFFER, 'the _DecodeLane (codec.py:1660): classified by DECODE_LANE'),
    'region': _entry(NOT_A_BUFFER, 'the crop size (rh, rw) of a RegionDecoder, None otherwise (codec.py:1661): a tuple'),
    'pinned_head': _entry(SCRATCH, 'plan_decode_step / plan_region_step writes every element of every field before the step is launched '
                                   '(codec.py:1418-1442, 2156-2173); the pad between fields is copied and never read'),
    'pinned_payload': _entry(SCRATCH, 'plan_decode_step / plan_region_step writes the bytes it announces (codec.py:1430, 1442; 2173-2176); the '
                                      'device fetches those'),
    'head_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_head (codec.py:1664)'),
    'payload_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_payload (codec.py:1664)'),
    'pinned_status': _entry(SCRATCH, 'publish_step copies all of the lane\'s `status` in front of the step counter (codec.py:1883)'),
    'results_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_status (codec.py:1666)'),
    'index_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_status (codec.py:1667)'),
    'pinned_unfinished': _entry(SCRATCH, 'publish_to_host copies the scratch block\'s status word every step (codec.py:1882)'),
    'unfinished_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_unfinished (codec.py:1669)'),
    'planes': _entry(SCRATCH, 'eae_hip_decode writes every pixel of every image, or window, of the step (codec.py:1880)'),
    'pinned_rec': _entry(SCRATCH, 'publish_to_host copies all of `planes` (codec.py:1913)'),
    'rec_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_rec (codec.py:1682)'),
    'crops': _entry(SCRATCH, 'publish_crops writes every 16-byte word of it: the rh x rw pixels of every crop of the batch, an absent one '
                             'from the origin plan_region_step left it (codec.py:2159), zeros behind the last (codec.py:2255; '
                             'codec_decode.hip:98-134); the ticket takes the present crops\' (codec.py:1697)'),
    'pinned_crops': _entry(SCRATCH, 'as `crops`, cut straight into pinned memory when the crops are fetched (codec.py:2255, 1679)'),
    'crops_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_crops (codec.py:1683)'),
    'seq_dev': _entry(CARRIED, 'step counter and publish_step\'s ticket word (codec.py:1684; misc.hip:133-138)'),
    'pinned_seq': _entry(CARRIED, 'the published counter the worker compares with `count` (codec.py:1685, 1837)'),
    'seq_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_seq (codec.py:1686)'),
    'count': _entry(CARRIED, 'how many times the host has submitted the slot (codec.py:1687, 1840): a Python int'),
    'free': _entry(NOT_A_BUFFER, 'a threading.Event (codec.py:1688)'),
    'graph': _entry(NOT_A_BUFFER, 'the torch.cuda.CUDAGraph of the slot\'s step; the captured step allocates nothing (codec.py:1873-1913, '
                                  '2243-2255 pass every output in)'),
}

for _table in (SLOT, DECODE_LANE):
    _table.update(_result_rows('coder_streams'))
    _table.update(_result_rows('classes[]'))
TABLES = {'_Slot': SLOT, '_DecodeLane': DECODE_LANE, '_DecodeSlot': DECODE_SLOT}

# What a reader might expect to be SCRATCH and must stay so: a test requires it (tests/test_slot_inventory.py).
MUST_BE_SCRATCH = {
    '_Slot': ('symbols', 'gathered', 'coder_streams.streams', 'classes[].streams', 'workspace', 'offsets', 'index', 'payload', 'exception_rows',
              'staging', 'graphs[1]', 'graphs[2]', 'graphs[3]', 'pinned_out', 'pinned_sse', 'pinned_payload', 'pinned_emit', 'pinned_rec',
              'pinned_symbols'),
    '_DecodeLane': ('head_bits', 'prob_row', 'placement', 'crop_origin', 'bin_widths', 'map_mean', 'table', 'payload_bytes', 'payload', 'results',
                    'index', 'offsets', 'coder_streams.streams', 'classes[].streams', 'workspace', 'symbols', 'decoded', 'shifted', 'scratch'),
    '_DecodeSlot': ('pinned_head', 'pinned_payload', 'pinned_status', 'pinned_unfinished', 'planes', 'pinned_rec', 'crops', 'pinned_crops'),
}


def attribute_of(name):
    """The attribute an entry belongs to: 'coder_streams.streams' -> 'coder_streams', 'classes[].rows' -> 'classes'."""
    for (k, c) in enumerate(name):
        if c in '.[':
            return name[:k]
    return name


def tensors_of(owner, table, name):
    """The tensors of entry `name` on the live object `owner` (none where the codec's mode leaves the attribute out or None)."""
    entry = table[name]
    found = entry.get(owner) if entry.get is not None else [getattr(owner, name, None)]
    return [t for t in found if isinstance(t, torch.Tensor)]


def scratch_leaves(owner, table):
    """[(name, tensor)]: every SCRATCH tensor of `owner`, each byte once (aliases are reached through what they are views of)."""
    return [(name, t) for (name, entry) in table.items() if entry.cls == SCRATCH and entry.alias is None for t in tensors_of(owner, table, name)]


def fill_bytes(tensor, byte):
    """Every byte of `tensor` (a view: its own elements only) becomes `byte`; on the current stream for a device tensor."""
    if tensor.numel():
        tensor.view(torch.uint8).fill_(int(byte))


def owners(codec_or_decoder):
    """[(object, table)] of every slot of a BatchCodec, or every slot and lane of a BatchDecoder or RegionDecoder."""
    out = []
    for slot in codec_or_decoder._slots:
        if hasattr(slot, 'lane'):
            out += [(slot, DECODE_SLOT), (slot.lane, DECODE_LANE)]
        else:
            out.append((slot, SLOT))
    return out


def poison_scratch(codec_or_decoder, byte):
    """Fills every SCRATCH buffer of every slot, device and pinned alike, through the leaf views only (CARRIED and CONSTANT bytes of
    the same storage stay). The codec must be idle (`drain()`); the device is synchronised behind the fills, because the codec's steps
    run on other streams than the one the fills went to. Returns the number of bytes filled."""
    total = 0
    for (owner, table) in owners(codec_or_decoder):
        for (_, tensor) in scratch_leaves(owner, table):
            fill_bytes(tensor, byte)
            total += tensor.numel()*tensor.element_size()
    torch.cuda.synchronize()
    return total


def _extent(tensor):
    assert tensor.is_contiguous(), 'a part of a container must be a contiguous view'
    return (tensor.data_ptr(), tensor.data_ptr() + tensor.numel()*tensor.element_size())


def check_tiling(owner, table):
    """Asserts, for every CONTAINER of `owner` that exists in this mode, that its parts lie inside it, do not overlap and leave no
    gap wider than the entry's `max_gap` bytes (alignment padding of `decode_head_layout`). Returns the containers checked."""
    checked = []
    for (name, entry) in table.items():
        if entry.cls != CONTAINER:
            continue
        whole = getattr(owner, name, None)
        if not isinstance(whole, torch.Tensor):
            continue
        (start, end) = _extent(whole)
        extents = sorted(_extent(t) for part in entry.parts for t in tensors_of(owner, table, part) if t.numel())
        assert extents, name
        position = start
        for (lo, hi) in extents:
            assert position <= lo <= position + entry.max_gap, '{0}: a part starts at byte {1}, the bytes before it end at {2}'.format(
                name, lo - start, position - start)
            position = hi
        assert position <= end <= position + entry.max_gap, '{0}: the parts end at byte {1} of {2}'.format(name, position - start, end - start)
        checked.append(name)
    return checked
