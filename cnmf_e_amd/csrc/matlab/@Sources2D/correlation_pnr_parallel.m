function [Cn, PNR] = correlation_pnr_parallel(obj, frame_range)
% CORRELATION_PNR_PARALLEL  drop-in for ca_source_extraction/@Sources2D/correlation_pnr_parallel.m on the MI355X engine: the local-correlation image
% Cn and the peak-to-noise image PNR of the spatially filtered video (endoscope/correlation_image_endoscope.m:36-96), per patch on the resident
% block (cnmfe_seed_images), the patch interiors put together as :108-128 do (they are disjoint: the reference's max is a plain assignment).
% Same arguments and results as the reference.  options.ssub / options.tsub other than 1 (:81-100): the block is down-sampled on the device
% (cnmfe_seed_images_ds: dsData), filtered with the kernel of gSig / ssub and ceil(gSiz / ssub), detrended against the basis of the floor(n / tsub)
% frames that are left, and with ssub > 1 both images are resized back here (imresize).  Not built (an error, as everywhere in this host):
% detrend_method 'local_min' with nk > 1, a frame range that does not start at frame 1.  Blocks are filtered whole: the 500^3-sample sub-patch split of
% correlation_image_endoscope.m:50-59 is a memory workaround of the host computation.
    eng = cnmfe_handle(obj);
    d1 = eng.dims(1);  d2 = eng.dims(2);  T = eng.dims(3);
    obj.options.d1 = d1;  obj.options.d2 = d2;
    if nargin < 2, frame_range = obj.frame_range; end
    if isempty(frame_range), frame_range = [1 T]; else, frame_range = min(max(frame_range, 1), T); end
    if frame_range(1) ~= 1, error('cnmfe:frame_range', 'the engine reads the frames from the first one on'); end
    opt = obj.options;
    need = {'gSig', 'gSiz', 'center_psf', 'ssub', 'tsub'};      % what the reference reads unconditionally (correlation_pnr_parallel.m:33-34, correlation_image_endoscope.m:22-37)
    for k = 1:numel(need)
        if ~isfield(opt, need{k}), error('cnmfe:options', 'correlation_pnr_parallel: options.%s is missing', need{k}); end
    end
    ssub = opt.ssub;  tsub = opt.tsub;
    if ssub ~= round(ssub) || ssub < 1 || ssub > 8, error('cnmfe:options', 'options.ssub must be an integer in 1..8, got %g', ssub); end
    if tsub ~= round(tsub) || tsub < 1, error('cnmfe:options', 'options.tsub must be an integer >= 1, got %g', tsub); end
    nk = 1;  if isfield(opt, 'nk'), nk = opt.nk; end
    if nk > 1 && ~(isfield(opt, 'detrend_method') && strcmpi(opt.detrend_method, 'spline'))
        error('cnmfe:unsupported', 'seed images: only detrend_method ''spline'' is built');
    end
    n = diff(frame_range) + 1;
    obj.frame_range = frame_range;
    ds = ssub ~= 1 || tsub ~= 1;
    Ts = floor(n / tsub);
    if ds && Ts < 64, error('cnmfe:options', 'options.tsub = %d leaves floor(%d / %d) = %d frames, at least 64 are needed', tsub, n, tsub, Ts); end
    psf = seed_psf(opt.gSig / ssub, ceil(opt.gSiz / ssub), opt.center_psf);      % :81-82
    Q = [];
    if nk > 1                                                   % detrend_data.m:23-29 is a projection: an orthonormal basis of the same span
        [Q, ~] = qr(full(bsplineM((1:Ts)', linspace(1, Ts, nk), 4)), 0);       % (of the down-sampled series, :86-93)
    end
    Cn = zeros(d1, d2);  PNR = zeros(d1, d2);
    for m = 1:numel(eng.pid)
        h = eng.h(eng.owner(m));
        p = eng.patch_pos{m};  b = eng.block_pos{m};
        if ds
            [cn_b, pnr_b] = cnmfe_mex('seed_images_ds', h, eng.pid(m), ssub, tsub, psf, n, Q);
            if ssub ~= 1                                        % :97-100
                cn_b = imresize(cn_b, [b(2) - b(1) + 1, b(4) - b(3) + 1]);
                pnr_b = imresize(pnr_b, [b(2) - b(1) + 1, b(4) - b(3) + 1]);
            end
        else
            [cn_b, pnr_b] = cnmfe_mex('seed_images', h, eng.pid(m), psf, n, Q);
        end
        rr = (p(1):p(2)) - b(1) + 1;  cc = (p(3):p(4)) - b(3) + 1;
        Cn(p(1):p(2), p(3):p(4)) = cn_b(rr, cc);
        PNR(p(1):p(2), p(3):p(4)) = pnr_b(rr, cc);
    end
end

function psf = seed_psf(gSig, gSiz, center_psf)
% the filter of correlation_image_endoscope.m:36-47; an even-sized kernel gets a leading zero row and column, which keeps imfilter's origin
% floor((n + 1) / 2) at the centre of the odd kernel the engine filters with
    if gSig <= 0, psf = []; return; end
    if center_psf
        psf = fspecial('gaussian', ceil(gSig * 4 + 1), gSig);
        keep = psf >= max(psf(:, 1));
        psf = psf - mean(psf(keep));
        psf(~keep) = 0;
    else
        psf = fspecial('gaussian', round(gSiz), gSig);
    end
    if mod(size(psf, 1), 2) == 0, psf = padarray(psf, [1 1], 0, 'pre'); end
end
