from transformer4sed_amd.ensemble import Score, ScoreContainer, score_average  # noqa: F401
