"""Mirror of the reference package layout (the supervised latent policy: ``model.Latent_Model``, ``train.Engine``)."""
