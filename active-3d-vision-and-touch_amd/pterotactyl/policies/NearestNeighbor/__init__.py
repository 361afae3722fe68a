"""Mirror of the reference package layout (the nearest-neighbour latent policy: ``train.Engine``, ``train.LatentBank``)."""
