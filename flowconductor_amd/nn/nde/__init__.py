from flowconductor_amd.nn.nde.made import MixtureOfGaussiansMADE  # noqa: F401
