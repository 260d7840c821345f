"""The trainers' photometric loss as the trainers write it -- Inria loss_utils.ssim: a 2-D window, F.conv2d(..., padding=5,
groups=3) -- in float64 torch, for torch.autograd to differentiate.  Independent of tests/photometric_loss_reference.py: it shares
no code with it, and tests/test_photometric_loss_api.py holds the one to the other."""
import torch
import torch.nn.functional as F


def gaussian(window_size=11, sigma=1.5):
    k = torch.arange(window_size, dtype=torch.float64)
    g = torch.exp(-((k - window_size // 2) ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def create_window(window_size=11, channels=3):
    g = gaussian(window_size).unsqueeze(1)
    return (g @ g.t()).unsqueeze(0).unsqueeze(0).expand(channels, 1, window_size, window_size).contiguous()


def ssim_map(img1, img2):
    """img: (3, H, W) float64."""
    window = create_window()
    img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    mu1 = F.conv2d(img1, window, padding=5, groups=3)
    mu2 = F.conv2d(img2, window, padding=5, groups=3)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=5, groups=3) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=5, groups=3) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=5, groups=3) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def loss_and_gradient(x, y, lam):
    """x, y: numpy float32 [H][W][3 or 4].  Returns (terms [loss, l1, ssim, mse], d loss / d x [H][W][3]) as float64 numpy."""
    img = torch.tensor(x[..., :3]).to(torch.float64).permute(2, 0, 1).contiguous().requires_grad_(True)
    gt = torch.tensor(y[..., :3]).to(torch.float64).permute(2, 0, 1).contiguous()
    l1 = (img - gt).abs().mean()
    mse = ((img - gt) ** 2).mean()
    if lam == 0:
        loss, ssim = l1, torch.tensor(float("nan"), dtype=torch.float64)
    else:
        ssim = ssim_map(img, gt).mean()
        loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    loss.backward()
    terms = torch.stack([loss.detach(), l1.detach(), ssim.detach(), mse.detach()]).numpy()
    return terms, img.grad.permute(1, 2, 0).contiguous().numpy()
