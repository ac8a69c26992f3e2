!> `initialize_many_clipped` of the drop-in module: a batch of a 1-D problem on 16 nodes, an empty problem and the first problem
!! again, xtrap = 1, klo = 2.5, khi = 3, up to 8 passes.  Checked here: the statuses, the outliers rejected, both copies with the same bits, maxpass = 0 with the bits of `initialize_many` and unit weights, the argument checks
!! and the refusal under set_host.  With two arguments the points come from a file (raw: int64 n, then n x and n y as doubles)
!! and coef, wout and clip go to a file (raw doubles) for a caller that compares the bits with another binding.
!!   usage: test_fit_many_clip [points.bin results.bin]
program test_fit_many_clip
    use splpak_module, wp => splpak_wp
    use, intrinsic :: iso_c_binding, only: c_int64_t, c_double
    implicit none
    integer,parameter :: nodes(1) = [16], ncol = 16, nbatch = 3, maxpass = 8
    real(wp),parameter :: xmin(1) = [0.0_wp], xmax(1) = [1.0_wp], klo = 2.5_wp, khi = 3.0_wp
    integer(c_int64_t) :: offsets(nbatch+1), n64
    real(wp),allocatable :: x(:,:), y(:), wout(:), w0(:)
    real(wp) :: coef(ncol,nbatch), c0(ncol,nbatch)
    real(c_double) :: clip(4,nbatch)
    integer :: ierrors(nbatch), ierror, ip, n, seed, nbad, u, nout
    character(len=1024) :: fin, fout
    type(splpak_type) :: s, h

    nbad = 0
    seed = 9173
    nout = 0
    if (command_argument_count() >= 2) then
        call get_command_argument(1, fin)
        call get_command_argument(2, fout)
        open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
        read(u) n64
        n = int(n64)
        allocate(x(1,2*n), y(2*n), wout(2*n), w0(2*n))
        read(u) x(1,1:n)
        read(u) y(1:n)
        close(u)
    else
        n = 300
        allocate(x(1,2*n), y(2*n), wout(2*n), w0(2*n))
        do ip = 1, n
            x(1,ip) = lcg()
            y(ip) = sin(3.0_wp*x(1,ip)) + 0.1_wp*(lcg() - 0.5_wp)
        end do
        nout = 6
        do ip = 1, nout      ! outliers of both signs at 20 times the noise
            y(40*ip) = y(40*ip) + merge(1.0_wp, -1.0_wp, mod(ip, 2) == 0)
        end do
    end if
    x(1,n+1:2*n) = x(1,1:n)
    y(n+1:2*n) = y(1:n)
    offsets = [0_c_int64_t, int(n,c_int64_t), int(n,c_int64_t), int(2*n,c_int64_t)]      ! problem 2 is empty

    coef = -7.0_wp
    wout = -5.0_wp
    call s%initialize_many_clipped(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, maxpass, wout, coef, ncol, &
                                   ierrors, ierror, clip=clip)
    if (ierror /= 105) then
        nbad = nbad + 1
        write(*,*) 'initialize_many_clipped: ierror ', ierror
    end if
    if (ierrors(1) /= 0 .or. ierrors(2) /= 105 .or. ierrors(3) /= 0) nbad = nbad + 1
    if (any(coef(:,2) /= -7.0_wp) .or. any(clip(:,2) /= 0.0_c_double)) nbad = nbad + 1
    if (any(coef(:,1) /= coef(:,3)) .or. any(wout(1:n) /= wout(n+1:2*n)) .or. any(clip(:,1) /= clip(:,3))) nbad = nbad + 1
    if (any(wout /= 0.0_wp .and. wout /= 1.0_wp)) nbad = nbad + 1
    if (nint(clip(2,1)) /= count(wout(1:n) == 0.0_wp) .or. nint(clip(3,1)) /= count(wout(1:n) /= 0.0_wp)) nbad = nbad + 1
    write(*,'(A,I3,A,I4,A,I4,A,ES12.4)') ' passes ', nint(clip(1,1)), ', rejected ', nint(clip(2,1)), ', counted ', nint(clip(3,1)), &
                                        ', v ', clip(4,1)
    if (nout > 0) then      ! the outliers are rejected
        if (nint(clip(2,1)) < nout .or. nint(clip(1,1)) < 2) nbad = nbad + 1
        do ip = 1, nout
            if (wout(40*ip) /= 0.0_wp) nbad = nbad + 1
        end do
    end if
    if (command_argument_count() >= 2) then
        open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
        write(u) coef
        write(u) wout
        write(u) clip
        close(u)
    end if

    ! maxpass = 0: the bits of initialize_many, unit weights out
    call s%initialize_many_clipped(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, 0, w0, c0, ncol, ierrors, ierror)
    if (ierror /= 105 .or. any(w0 /= 1.0_wp)) nbad = nbad + 1
    coef = -7.0_wp
    call s%initialize_many(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, coef, ncol, ierrors, ierror)
    if (ierror /= 105 .or. any(coef(:,1) /= c0(:,1)) .or. any(coef(:,3) /= c0(:,3))) nbad = nbad + 1
    ! the argument checks are the library's; under set_host the entry refuses
    call s%initialize_many_clipped(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, 0.5_wp, khi, maxpass, wout, coef, ncol, &
                                   ierrors, ierror)
    if (ierror /= -3) nbad = nbad + 1
    call s%initialize_many_clipped(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, -1, wout, coef, ncol, ierrors, ierror)
    if (ierror /= -3) nbad = nbad + 1
    call h%set_host(.true.)
    call h%initialize_many_clipped(1, nbatch, offsets, x, 1, y, xmin, xmax, nodes, 1.0_wp, klo, khi, maxpass, wout, coef, ncol, &
                                   ierrors, ierror)
    if (ierror /= -4) nbad = nbad + 1
    if (nbad /= 0) error stop 'FAIL test_fit_many_clip'
    write(*,'(A)') ' PASS test_fit_many_clip'
contains
    real(wp) function lcg()
        seed = mod(seed*1103 + 12345, 65536)
        lcg = real(seed, wp)/65536.0_wp
    end function lcg
end program test_fit_many_clip
