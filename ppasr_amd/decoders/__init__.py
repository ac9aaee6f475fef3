from ppasr_amd.decoders.ctc_alignment import ctc_align_ids, forced_align  # noqa: F401
