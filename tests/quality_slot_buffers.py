"""What every buffer of `codec._QualitySlot` may hold when a `QualityCodec` step starts: the table of tests/ratecontrol_slot_buffers.py for
this member of the slot family (a plain helper module: import it, no fixture lives here). tests/test_quality_rule_host.py keeps the table
complete; tests/test_gpu_quality_codec_slots.py poisons the SCRATCH entries between steps, together with `_Slot`'s."""
import ratecontrol_slot_buffers
from ratecontrol_slot_buffers import slots_of as quality_slots      # noqa: F401 (the `_QualitySlot` of every slot of a codec, in the slots' order)

QUALITY_SLOT = ratecontrol_slot_buffers.slot_table(tiled=False, quality=True)
MUST_BE_SCRATCH = ratecontrol_slot_buffers.must_be_scratch(quality=True)


def poison_scratch(codec, byte):
    """`ratecontrol_slot_buffers.poison_scratch` with this table."""
    return ratecontrol_slot_buffers.poison_scratch(codec, QUALITY_SLOT, byte)
