from ppasr_amd.decoders.ctc_alignment import ctc_align_ids, forced_align  # noqa: F401
from ppasr_amd.decoders.attention_decoder import attention_decode  # noqa: F401
