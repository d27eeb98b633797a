from .pileup import apa_scores, pileup_from_sums, pileup_pixels, shifted_controls  # noqa: F401
