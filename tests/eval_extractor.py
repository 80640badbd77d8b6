"""TEST INFRASTRUCTURE: a deterministic feature extractor for gan_variant_research_amd.evaluate, in torch: average-pool the uint8
(B, 3, S, S) batch to 8 x 8, then a seeded 192 -> 40 projection with a ReLU.  `--extractor tests.eval_extractor:make` names it on the
command line.  Never imported by the product package."""
import torch

D_IN, D_OUT, SEED = 3 * 8 * 8, 40, 20240


def make(device):
    g = torch.Generator().manual_seed(SEED)
    W = (torch.randn(D_IN, D_OUT, generator=g, dtype=torch.float64) / D_IN ** 0.5).to(device)
    bias = torch.linspace(-0.5, 0.5, D_OUT, dtype=torch.float64).to(device)

    def extract(u8: torch.Tensor) -> torch.Tensor:
        assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[1] == 3
        x = torch.nn.functional.adaptive_avg_pool2d(u8.to(torch.float64) / 255.0 - 0.5, 8).reshape(u8.shape[0], D_IN)
        return torch.relu(x.to(W.device) @ W + bias).float()

    return extract
