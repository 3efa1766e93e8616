"""Model constructors of the hot path (same names / signatures / module layout as
pytorch_generative.models: models.autoregressive.<module>, models.vae.<module>, models.kde, models.mixture_models; NICE lives
in models.flows.nice — `flows`, plural, and no top-level models.NICE: under the drop-in alias the reference's names `models.flow`
and `models.NICE` keep their raising placeholders, compat.py; the Gaussian process lives in models.gaussian_process and, as in the
reference, has no top-level name)."""

from pytorch_generative_amd.models import autoregressive, base, flows, gaussian_process, kde, mixture_models, vae  # noqa: F401
from pytorch_generative_amd.models.autoregressive.gated_pixel_cnn import GatedPixelCNN
from pytorch_generative_amd.models.autoregressive.image_gpt import ImageGPT
from pytorch_generative_amd.models.autoregressive.made import MADE
from pytorch_generative_amd.models.autoregressive.pixel_cnn import PixelCNN
from pytorch_generative_amd.models.autoregressive.pixel_cnn_pp import PixelCNNpp
from pytorch_generative_amd.models.autoregressive.pixel_snail import PixelSNAIL
from pytorch_generative_amd.models.kde import GaussianKernel, KernelDensityEstimator, ParzenWindowKernel
from pytorch_generative_amd.models.mixture_models import BernoulliMixtureModel, GaussianMixtureModel
from pytorch_generative_amd.models.vae.beta_vae import BetaVAE
from pytorch_generative_amd.models.vae.vae import VAE
from pytorch_generative_amd.models.vae.vd_vae import VeryDeepVAE
from pytorch_generative_amd.models.vae.vq_vae import VectorQuantizedVAE
from pytorch_generative_amd.models.vae.vq_vae_2 import VectorQuantizedVAE2

__all__ = ["GatedPixelCNN", "ImageGPT", "MADE", "PixelCNN", "PixelCNNpp", "PixelSNAIL", "VAE", "BetaVAE", "VeryDeepVAE",
           "VectorQuantizedVAE", "VectorQuantizedVAE2", "KernelDensityEstimator", "GaussianKernel", "ParzenWindowKernel",
           "GaussianMixtureModel", "BernoulliMixtureModel"]
