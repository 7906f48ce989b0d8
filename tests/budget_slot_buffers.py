"""What every buffer of `codec._BudgetSlot` may hold when a `BudgetCodec` step starts: tests/slot_buffers.py's classification for the
state a step owns beyond its `_Slot` (a plain helper module: import it, no fixture lives here). tests/test_budget_rule_host.py keeps
the table complete; tests/test_gpu_budget_codec.py poisons the SCRATCH entries between steps, together with `_Slot`'s.

The reasons name lines of codec.py (`BudgetCodec._launch_analysis`, `_launch_coder`, `_stage`), device.py and csrc/hip/budget.hip as
of the commit that last touched the entry. For every SCRATCH entry the reason names the launch (or host write) of the SAME step that
defines it in front of its first reader."""
import torch

import slot_buffers
from slot_buffers import CARRIED, CONSTANT, CONTAINER, NOT_A_BUFFER, SCRATCH, _entry      # noqa: F401 (CARRIED: no entry needs it)

_ZEROED = ('`accum.zero_()` is the first launch of the step (codec.py:2500) and covers all of `accum`; ladder_kernel then adds into it '
           '(codec.py:2507; ladder.hip:79, 84), in front of ladder_select_kernel, its only reader (codec.py:2510)')
_SELECTED = ('ladder_select_kernel writes every element on every call (budget.hip:100-106; codec.py:2510) in front of its readers: '
             'latent_rows_kernel, the coder and the publication (codec.py:2516, 2535, 2543)')

BUDGET_SLOT = {
    'accum': _entry(CONTAINER, 'codec.py:2337: [bypass bits | histograms | range errors], zeroed as one',
                    parts=('bypass_bits', 'hist', 'range_errors')),
    'bypass_bits': _entry(SCRATCH, _ZEROED),
    'hist': _entry(SCRATCH, _ZEROED),
    'range_errors': _entry(SCRATCH, _ZEROED + '; nothing reads it: a point with range errors shows as an incomplete histogram (budget.hip:92)'),
    'pinned_budgets': _entry(SCRATCH, '`BudgetCodec._stage` writes the batch_size budgets of the step before its first launch (codec.py:2481); the '
                                      'pad word of an odd batch is copied and never read (codec.py:2511 passes budgets[:batch_size])'),
    'budgets_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_budgets (codec.py:2344)'),
    'budgets': _entry(SCRATCH, 'fetch_prefix copies budgets_nbytes = ALL of pinned_budgets (codec.py:2509) in front of ladder_select_kernel '
                               '(codec.py:2510)'),
    'budgets_nbytes': _entry(CONSTANT, 'the size of the budget block, written at construction (codec.py:2346), read by fetch_prefix'),
    'select': _entry(CONTAINER, 'codec.py:2348: [upper | point | flags], published as one', parts=('upper', 'point', 'flags')),
    'upper': _entry(SCRATCH, _SELECTED),
    'point': _entry(SCRATCH, _SELECTED),
    'flags': _entry(SCRATCH, _SELECTED),
    'prob_row': _entry(SCRATCH, _SELECTED),
    'pinned_select': _entry(SCRATCH, 'publish_to_host copies all of `select` in front of the coder side\'s step counter (codec.py:2543, 2546)'),
    'select_host': _entry(NOT_A_BUFFER, 'numpy views of pinned_select (codec.py:2363)'),
    'table': _entry(CONTAINER, 'codec.py:2356: [the K x 128 rows of the ladder | one row per image]', parts=('points_table', 'exception_rows')),
    'points_table': _entry(CONSTANT, 'the ladder\'s probability rows, copied at construction (codec.py:2358) and only read by the coder'),
    'exception_rows': _entry(SCRATCH, 'with an exception map exception_rows_kernel writes all L entries of every image\'s row in front of the '
                                      'coder (codec.py:2534; codec_container.hip:218); without one no prob_row names them (budget.hip:106) and '
                                      'the worker takes none (codec.py:2392)'),
    'pinned_rows': _entry(SCRATCH, 'with an exception map publish_to_host copies all of exception_rows in front of the step counter '
                                   '(codec.py:2545); without one the worker does not read it (codec.py:2392)'),
    'rows_host': _entry(NOT_A_BUFFER, 'numpy view of pinned_rows (codec.py:2361)'),
}

MUST_BE_SCRATCH = ('bypass_bits', 'hist', 'range_errors', 'pinned_budgets', 'budgets', 'upper', 'point', 'flags', 'prob_row', 'pinned_select',
                   'exception_rows', 'pinned_rows')


def budget_slots(codec):
    """The `_BudgetSlot` of every slot of a `BudgetCodec`, in the slots' order."""
    return [codec._budget_slots[id(slot)] for slot in codec._slots]


def poison_scratch(codec, byte):
    """Fills every SCRATCH buffer of every `_BudgetSlot`, device and pinned alike (`slot_buffers.poison_scratch` does the `_Slot`s).
    The codec must be idle. Returns the number of bytes filled."""
    total = 0
    for owner in budget_slots(codec):
        for (_, tensor) in slot_buffers.scratch_leaves(owner, BUDGET_SLOT):
            slot_buffers.fill_bytes(tensor, byte)
            total += tensor.numel()*tensor.element_size()
    torch.cuda.synchronize()
    return total
