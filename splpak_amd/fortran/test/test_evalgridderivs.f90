!> `evaluate_grid_derivatives` of the drop-in module against its own scalar `evaluate` (the host computation that
!! test_evalfix holds to the reference's splde values, src/splpak.F90:1089-1240): EVERY plane -- value, gradient and, for
!! order 2, the upper triangle of the Hessian -- at EVERY point of a tensor-product grid of points, under the matching
!! nderiv, on the node grids and coefficients of the golden fixtures tests/golden/eval_<case>.txt (only their headers and
!! coefficients are read).  Axes as in test_evalgrid: unsorted, with xmin, xmax, a node position, a repeated value and
!! points outside the box.  f has three rows more than there are grid points; they must keep their contents.
!! With `host` as first argument the object runs under set_host(.true.) and the bar is 1e-12 (no GPU needed); without it
!! the call runs on the GPU (more than four dimensions: on the host, by the module itself) and the bar is 1e-10.
!!   usage: test_evalgridderivs [host] <fixture.txt> [...]
program test_evalgridderivs
    use splpak_module, wp => splpak_wp
    implicit none
    integer :: nargs, ia, nbad, first
    logical :: host
    real(wp) :: tol
    character(len=1024) :: path

    nbad = 0
    host = .false.
    first = 1
    nargs = command_argument_count()
    if (nargs >= 1) then
        call get_command_argument(1, path)
        if (trim(path) == 'host') then
            host = .true.
            first = 2
        end if
    end if
    if (nargs < first) error stop 'usage: test_evalgridderivs [host] fixture.txt ...'
    tol = merge(1.0e-12_wp, 1.0e-10_wp, host)
    do ia = first, nargs
        call get_command_argument(ia, path)
        call one(trim(path))
    end do
    if (nbad /= 0) error stop 'FAIL test_evalgridderivs'
    write(*,'(A)') ' PASS test_evalgridderivs'
contains
    subroutine one(file)
        character(len=*),intent(in) :: file
        integer :: u, ndim, ncol, npat, nqf, k, j, ierror, seed, iq, nq, idim, order, nplanes, col, d1, d2, ldf, nchecked
        integer :: nodes(8), npts(8), nder(8), off(8), kk(8)
        real(wp) :: xmin(8), xmax(8), x(8), w, v, vmax, worst, cmax, scale
        real(wp),parameter :: guard = -12345.0_wp
        real(wp),allocatable :: coef(:), axes(:), f(:,:), fs(:)
        type(splpak_type) :: s
        open(newunit=u, file=file, status='old', action='read')
        read(u,*) ndim
        read(u,*) nodes(1:ndim)
        read(u,*) xmin(1:ndim)
        read(u,*) xmax(1:ndim)
        read(u,*) ncol, npat, nqf
        allocate(coef(ncol))
        do k = 1, ncol
            read(u,*) coef(k)
        end do
        close(u)
        if (host) call s%set_host(.true.)
        call s%destroy(ndim)
        ! odd counts, more points along the first dimensions; small in 5-D
        do k = 1, ndim
            npts(k) = merge(11 - 2*k, 4 + mod(k,2), ndim <= 4)
        end do
        if (ndim == 3) npts(1) = 70             ! more than one workgroup tile along the first dimension
        nq = product(npts(1:ndim))
        ldf = nq + 3
        allocate(axes(sum(npts(1:ndim))), fs(nq))
        seed = 12345 + ndim
        j = 0
        do k = 1, ndim
            off(k) = j
            w = xmax(k) - xmin(k)
            do iq = 1, npts(k)
                seed = mod(seed*1103 + 12345, 65536)
                axes(j+iq) = xmin(k) - 0.15_wp*w + 1.3_wp*w*real(seed,wp)/65536.0_wp
            end do
            axes(j+1) = xmax(k)
            axes(j+2) = xmin(k) + (w/real(nodes(k)-1,wp))*real(nodes(k)/2,wp)     ! a node
            axes(j+npts(k)) = xmin(k)
            if (npts(k) >= 5) axes(j+4) = axes(j+3)                               ! a repeat
            j = j + npts(k)
        end do
        cmax = maxval(abs(coef))
        worst = 0.0_wp
        nchecked = 0
        do order = 1, 2
            nplanes = 1 + ndim + merge(ndim*(ndim+1)/2, 0, order == 2)
            allocate(f(ldf,nplanes))
            f = guard
            call s%evaluate_grid_derivatives(ndim, npts(1:ndim), axes, order, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), &
                                             f, ldf, ierror)
            if (ierror /= 0) then
                nbad = nbad + 1
                write(*,*) 'ierror ', ierror, ' order ', order
            end if
            d1 = 1
            d2 = 0
            do col = 1, nplanes
                ! the pattern of this plane: the entries of evaluate_derivatives in their order
                nder = 0
                if (col > 1 .and. col <= 1 + ndim) then
                    nder(col-1) = 1
                else if (col > 1 + ndim) then
                    d2 = d2 + 1
                    if (col == 2 + ndim) d2 = 1
                    if (d2 > ndim) then
                        d1 = d1 + 1
                        d2 = d1
                    end if
                    nder(d1) = nder(d1) + 1
                    nder(d2) = nder(d2) + 1
                end if
                ! the scalar evaluation at every grid point, dimension 1 fastest
                kk = 1
                vmax = 0.0_wp
                do iq = 1, nq
                    do idim = 1, ndim
                        x(idim) = axes(off(idim) + kk(idim))
                    end do
                    fs(iq) = s%evaluate(ndim, x(1:ndim), nder(1:ndim), coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), ierror)
                    if (ierror /= 0) nbad = nbad + 1
                    vmax = max(vmax, abs(fs(iq)))
                    idim = 1
                    do while (idim <= ndim)
                        kk(idim) = kk(idim) + 1
                        if (kk(idim) <= npts(idim)) exit
                        kk(idim) = 1
                        idim = idim + 1
                    end do
                end do
                ! scale = the size of the terms that are summed (as test_evalfix)
                scale = cmax
                do k = 1, ndim
                    scale = scale * (real(nodes(k) - 1, wp)/(xmax(k) - xmin(k)))**nder(k)
                end do
                vmax = max(vmax, scale)
                do iq = 1, nq
                    v = abs(f(iq,col) - fs(iq))
                    worst = max(worst, v/max(vmax, tiny(1.0_wp)))
                    if (.not. (v <= tol*vmax)) then
                        nbad = nbad + 1
                        if (nbad < 10) write(*,'(A,I2,A,I3,A,I8,2ES25.16)') ' mismatch: order ', order, ' plane ', col, &
                                                                           ' point ', iq, f(iq,col), fs(iq)
                    end if
                end do
                if (any(f(nq+1:ldf,col) /= guard)) then
                    nbad = nbad + 1
                    write(*,*) 'rows beyond the grid points were written: order ', order, ' plane ', col
                end if
                nchecked = nchecked + 1
            end do
            deallocate(f)
        end do
        ! the argument checks of the module / the library: -3
        allocate(f(ldf,1+ndim))
        call s%evaluate_grid_derivatives(ndim, npts(1:ndim), axes, 3, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), f, ldf, ierror)
        if (ierror /= -3) nbad = nbad + 1
        call s%evaluate_grid_derivatives(ndim, npts(1:ndim), axes, 1, coef, xmin(1:ndim), xmax(1:ndim), nodes(1:ndim), f, nq-1, ierror)
        if (ierror /= -3) nbad = nbad + 1
        write(*,'(A,A,A,I4,A,I8,A,ES10.2)') ' ', file, ': ', nchecked, ' planes x ', nq, ' grid points, worst relative difference ', worst
    end subroutine one
end program test_evalgridderivs
