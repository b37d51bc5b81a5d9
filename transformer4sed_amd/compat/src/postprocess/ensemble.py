from transformer4sed_amd.ensemble import ensemble, load_predictions, save_predictions, weighted_average_ensemble  # noqa: F401
