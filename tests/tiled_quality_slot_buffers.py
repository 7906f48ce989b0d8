"""What every buffer of `codec._TiledQualitySlot` may hold when a `TiledQualityCodec` step starts: tests/slot_buffers.py's
classification for the state a step owns beyond its `_Slot` (a plain helper module: import it, no fixture lives here).
tests/test_tiled_quality_host.py keeps the table complete; tests/test_gpu_tiled_quality_codec_slots.py poisons the SCRATCH entries
between steps, together with `_Slot`'s.

The reasons name the function of codec.py, device.py or csrc/hip the entry rests on, and the step of DESIGN.md section 22's launch
list (1 to 14) it is defined in: for every SCRATCH entry the launch (or host write) of the SAME step that defines it in front of its
first reader."""
import torch

import slot_buffers
from slot_buffers import CARRIED, CONSTANT, CONTAINER, NOT_A_BUFFER, SCRATCH, _entry      # noqa: F401 (CARRIED: no entry needs it)

_ZEROED = ('step 1: `accum.zero_()` is the first launch of `BudgetCodec._launch_selection` and covers all of `accum`; step 3: '
           'ladder_tiles_kernel then adds into it (ladder.hip), in front of ladder_select_tiles_kernel, its only reader (step 5)')
_SELECTED = ('step 5: ladder_select_tiles_kernel writes every element on every call (budget.hip; `TiledQualityCodec._launch_select` hands '
             'it `first` as its point) in front of its readers: quality_search_tiles_kernel (steps 7, 9) and the publication (step 14)')
_ROUND_0 = ('step 7: round 0 of quality_search_tiles_kernel writes every element of every output (quality.hip: search_round, thread 0 of '
            'every image\'s block) in front of the first probe (step 8); ')

TILED_QUALITY_SLOT = {
    'accum': _entry(CONTAINER, '`_TiledQualitySlot.__init__`: [bypass bits | histograms | range errors] of N x K x T x 128 streams, zeroed as one',
                    parts=('bypass_bits', 'hist', 'range_errors')),
    'bypass_bits': _entry(SCRATCH, _ZEROED),
    'hist': _entry(SCRATCH, _ZEROED),
    'range_errors': _entry(SCRATCH, _ZEROED + '; nothing reads it: a point with range errors shows as an incomplete histogram (s_count, budget.hip)'),
    'pinned_budgets': _entry(SCRATCH, '`QualityCodec._stage` writes the batch_size budgets of the step before its first launch (2^62 without '
                                      'a budget); the pad word of an odd batch is copied and never read (step 5 passes budgets[:batch_size])'),
    'budgets_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_budgets'),
    'budgets': _entry(SCRATCH, 'step 4: fetch_prefix copies budgets_nbytes = ALL of pinned_budgets in front of ladder_select_tiles_kernel (step 5)'),
    'budgets_nbytes': _entry(CONSTANT, 'the size of the budget block (8 bytes per image, padded to 16), written at construction, read by fetch_prefix'),
    'pinned_max_sse': _entry(SCRATCH, '`QualityCodec._stage` writes the batch_size thresholds of the step before its first launch; the pad word '
                                      'of an odd batch is copied and never read (`_launch_round` passes max_sse[:batch_size])'),
    'max_sse_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_max_sse'),
    'max_sse': _entry(SCRATCH, 'step 6: fetch_prefix copies max_sse_nbytes = ALL of pinned_max_sse in front of round 1 of '
                               'quality_search_tiles_kernel, its first reader (step 9; round 0 does not read it)'),
    'max_sse_nbytes': _entry(CONSTANT, 'the size of the threshold block, written at construction, read by fetch_prefix'),
    'select': _entry(CONTAINER, '`_TiledQualitySlot.__init__`: [upper | first | flags | trace_sse | point | met | state | trace_point], published '
                                'as one', parts=('upper', 'first', 'flags', 'trace_sse', 'point', 'met', 'state', 'trace_point')),
    'upper': _entry(SCRATCH, _SELECTED),
    'first': _entry(SCRATCH, _SELECTED),
    'flags': _entry(SCRATCH, _SELECTED),
    'trace_sse': _entry(SCRATCH, _ROUND_0 + '-1 everywhere, then round r writes column r - 1 (step 9)'),
    'trace_point': _entry(SCRATCH, _ROUND_0 + '-1 everywhere, then round r writes column r - 1 (step 9)'),
    'point': _entry(SCRATCH, _ROUND_0 + 'every round writes it again in front of the quantiser that reads it (steps 8, 10)'),
    'met': _entry(SCRATCH, _ROUND_0 + 'every round writes it again, the last one the answer'),
    'state': _entry(SCRATCH, _ROUND_0 + 'round r >= 1 reads what round r - 1 of the same step wrote'),
    'prob_row': _entry(SCRATCH, 'step 5: tile_prob_rows_kernel writes all n_streams = entries x 128 rows, and so does every round of '
                                'quality_search_tiles_kernel (steps 7, 9: `run_entry` is a permutation of the entries, each image\'s block '
                                'writes its own T), the last one in front of the coder\'s batches (step 12)'),
    'class_rows': _entry(SCRATCH, 'views of `prob_row`, one per shape class (`coding_tile_layout`\'s runs cover all n_streams)', alias='prob_row'),
    'pinned_select': _entry(SCRATCH, 'step 14: publish_to_host copies all of `select` in front of the coder side\'s step counter '
                                     '(`BudgetCodec._publish_coder_side`)'),
    'select_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select: upper, first, flags'),
    'search_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select: point, met, trace_point, trace_sse'),
    'probe_acc': _entry(SCRATCH, _ROUND_0 + '0; tconv3_kernel of a probe adds the squared errors (step 8), the round behind it reads and zeroes '
                                            'them (step 9)'),
    'probe_latent': _entry(SCRATCH, 'step 8: latent_rows_kernel writes every latent of every image (t_out, or shifted_out of the learned model) '
                                    'in front of the probe\'s tconv1, its only reader'),
    'table': _entry(CONTAINER, '`_TiledQualitySlot.__init__`: [the K x 128 rows of the ladder | one row per image]',
                    parts=('points_table', 'exception_rows')),
    'points_table': _entry(CONSTANT, 'the ladder\'s K x 128 probability rows, copied at construction and only read by the coder'),
    'exception_rows': _entry(SCRATCH, 'step 11: with an exception map exception_rows_kernel writes all L entries of every image\'s row in front '
                                      'of the coder (codec_container.hip); without one no prob_row names them (quality_search_tiles_kernel: '
                                      'idx_exception = -1 matches no map) and the worker takes none (`_QualityWorker._finish`)'),
    'pinned_rows': _entry(SCRATCH, 'step 14: with an exception map publish_to_host copies all of exception_rows in front of the step counter; '
                                   'without one the worker does not read it (`_QualityWorker._finish`: idx_map_exception < 0)'),
    'rows_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_rows'),
}

MUST_BE_SCRATCH = ('bypass_bits', 'hist', 'range_errors', 'pinned_budgets', 'budgets', 'pinned_max_sse', 'max_sse', 'upper', 'first', 'flags',
                   'trace_sse', 'trace_point', 'point', 'met', 'state', 'prob_row', 'pinned_select', 'probe_acc', 'probe_latent',
                   'exception_rows', 'pinned_rows')


def quality_slots(codec):
    """The `_TiledQualitySlot` of every slot of a `TiledQualityCodec`, in the slots' order."""
    return [codec._budget_slots[id(slot)] for slot in codec._slots]


def poison_scratch(codec, byte):
    """Fills every SCRATCH buffer of every `_TiledQualitySlot`, device and pinned alike (`slot_buffers.poison_scratch` does the
    `_Slot`s). The codec must be idle. Returns the number of bytes filled."""
    total = 0
    for owner in quality_slots(codec):
        for (_, tensor) in slot_buffers.scratch_leaves(owner, TILED_QUALITY_SLOT):       # (`class_rows`: through `prob_row`)
            slot_buffers.fill_bytes(tensor, byte)
            total += tensor.numel()*tensor.element_size()
    torch.cuda.synchronize()
    return total
