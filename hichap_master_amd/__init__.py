from .pileup import apa_scores, pileup_from_sums, pileup_pixels, shifted_controls  # noqa: F401
from .domain_pileup import domain_pileup_from_sums, domain_pileup_pixels, domain_scores  # noqa: F401
