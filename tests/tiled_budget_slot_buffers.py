"""What every buffer of `codec._TiledBudgetSlot` may hold when a `TiledBudgetCodec` step starts: tests/slot_buffers.py's
classification for the state a step owns beyond its `_Slot` (a plain helper module: import it, no fixture lives here).
tests/test_tiled_budget_rule_host.py keeps the table complete; tests/test_gpu_tiled_budget_codec.py poisons the SCRATCH entries
between steps, together with `_Slot`'s.

The reasons name the function of codec.py, device.py or csrc/hip the entry rests on, and the step of DESIGN.md section 20's table
(1 to 13) it is defined in: for every SCRATCH entry the launch (or host write) of the SAME step that defines it in front of its first
reader."""
import torch

import slot_buffers
from slot_buffers import CARRIED, CONSTANT, CONTAINER, NOT_A_BUFFER, SCRATCH, _entry      # noqa: F401 (CARRIED: no entry needs it)

_ZEROED = ('step 1: `accum.zero_()` is the first launch of `BudgetCodec._launch_analysis` and covers all of `accum`; step 3: '
           'ladder_tiles_kernel then adds into it (ladder.hip), in front of ladder_select_tiles_kernel, its only reader (step 5)')
_SELECTED = ('step 5: ladder_select_tiles_kernel writes every element on every call (budget.hip: point and flags by thread 0, upper by '
             'the first K threads of every image\'s block) in front of its readers: latent_rows_kernel (step 6), tile_prob_rows_kernel and '
             'the publication (step 13)')

TILED_BUDGET_SLOT = {
    'accum': _entry(CONTAINER, '`_TiledBudgetSlot.__init__`: [bypass bits | histograms | range errors] of N x K x T x 128 streams, zeroed as one',
                    parts=('bypass_bits', 'hist', 'range_errors')),
    'bypass_bits': _entry(SCRATCH, _ZEROED),
    'hist': _entry(SCRATCH, _ZEROED),
    'range_errors': _entry(SCRATCH, _ZEROED + '; nothing reads it: a point with range errors shows as an incomplete histogram (s_count, budget.hip)'),
    'pinned_budgets': _entry(SCRATCH, '`BudgetCodec._stage` writes the batch_size budgets of the step before its first launch; the pad word '
                                      'of an odd batch is copied and never read (step 5 passes budgets[:batch_size])'),
    'budgets_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_budgets'),
    'budgets': _entry(SCRATCH, 'step 4: fetch_prefix copies budgets_nbytes = ALL of pinned_budgets in front of ladder_select_tiles_kernel (step 5)'),
    'budgets_nbytes': _entry(CONSTANT, 'the size of the budget block (8 bytes per image, padded to 16), written at construction, read by fetch_prefix'),
    'select': _entry(CONTAINER, '`_TiledBudgetSlot.__init__`: [upper | point | flags], published as one', parts=('upper', 'point', 'flags')),
    'upper': _entry(SCRATCH, _SELECTED),
    'point': _entry(SCRATCH, _SELECTED),
    'flags': _entry(SCRATCH, _SELECTED),
    'prob_row': _entry(SCRATCH, 'step 5: tile_prob_rows_kernel, the second launch of eae_hip_ladder_select_tiles, writes all n_streams = entries '
                                'x 128 rows (budget.hip) in front of the coder\'s batches (step 10)'),
    'class_rows': _entry(SCRATCH, 'views of `prob_row`, one per shape class (`coding_tile_layout`\'s runs cover all n_streams)', alias='prob_row'),
    'pinned_select': _entry(SCRATCH, 'step 13: publish_to_host copies all of `select` in front of the coder side\'s step counter '
                                     '(`BudgetCodec._publish_coder_side`)'),
    'select_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select'),
    'table': _entry(CONTAINER, '`_TiledBudgetSlot.__init__`: [the K x 128 rows of the ladder | one row per image]',
                    parts=('points_table', 'exception_rows')),
    'points_table': _entry(CONSTANT, 'the ladder\'s K x 128 probability rows, copied at construction and only read by the coder'),
    'exception_rows': _entry(SCRATCH, 'step 8: with an exception map exception_rows_kernel writes all L entries of every image\'s row in front of '
                                      'the coder (codec_container.hip); without one no prob_row names them (tile_prob_rows_kernel: idx_exception '
                                      '= -1 matches no map) and the worker takes none (`_BudgetWorker._finish`)'),
    'pinned_rows': _entry(SCRATCH, 'step 13: with an exception map publish_to_host copies all of exception_rows in front of the step counter; '
                                   'without one the worker does not read it (`_BudgetWorker._finish`: idx_map_exception < 0)'),
    'rows_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_rows'),
}

MUST_BE_SCRATCH = ('bypass_bits', 'hist', 'range_errors', 'pinned_budgets', 'budgets', 'upper', 'point', 'flags', 'prob_row', 'pinned_select',
                   'exception_rows', 'pinned_rows')


def budget_slots(codec):
    """The `_TiledBudgetSlot` of every slot of a `TiledBudgetCodec`, in the slots' order."""
    return [codec._budget_slots[id(slot)] for slot in codec._slots]


def poison_scratch(codec, byte):
    """Fills every SCRATCH buffer of every `_TiledBudgetSlot`, device and pinned alike (`slot_buffers.poison_scratch` does the
    `_Slot`s). The codec must be idle. Returns the number of bytes filled."""
    total = 0
    for owner in budget_slots(codec):
        for (_, tensor) in slot_buffers.scratch_leaves(owner, TILED_BUDGET_SLOT):        # (`class_rows`: through `prob_row`)
            slot_buffers.fill_bytes(tensor, byte)
            total += tensor.numel()*tensor.element_size()
    torch.cuda.synchronize()
    return total
