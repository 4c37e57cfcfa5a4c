"""The paper's comparison baselines -- counterpart of the reference's footprints/baselines/ (SURVEY.md section 2 row 16)."""
